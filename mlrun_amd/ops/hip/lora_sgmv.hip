// Copyright 2026 mlrun_amd authors
//
// Licensed under the Apache License, Version 2.0 (the "License");
// you may not use this file except in compliance with the License.
//
// Multi-LoRA prefill: segmented gather mat-mul (SGMV) pair on
// v_mfma_f32_16x16x32_bf16 for gfx950.
//
// The token rows of a packed prefill are grouped by adapter on the host
// into a tile table, int32 [ntiles, 3] = (row0, nrows, adapter): at most
// 16 consecutive rows of ONE adapter per tile, base-model rows in no
// tile at all.  With the tables A [NA, R, K] and Bm [NA, N, R] (bf16;
// alpha / r folded into Bm at load time) the two kernels compute, for the
// rows r of a tile of adapter a,
//   shrink: t[r, j] = sum_k x[r, k] * A[a, j, k]                   (f32)
//   expand: y[r, n] = bf16(float(y[r, n]) + sum_j t[r, j] * Bm[a, n, j])
// the contract of the decode pair lora_shrink / lora_expand.
//
// Both kernels are total: a tile whose adapter is outside [0, NA), whose
// nrows is outside [1, 16] or whose rows leave [0, T) is skipped, and
// the test is block-uniform and comes before any barrier.  Rows, columns
// and k-slots past an edge are clamped on load (the address stays inside
// the tile's own rows and the adapter's own table slot) and never stored,
// so rows of x / t / y that no tile covers and table slots that no tile
// names are neither read nor written.  Every output has one owner and one
// summation order, fixed by (K, R) alone: no atomics, and a row's result
// does not depend on which other rows, tiles or adapters share the call.
// Capture-safe: no allocation, no sync.

#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.h"

typedef __attribute__((ext_vector_type(8))) short short8v;
typedef __attribute__((ext_vector_type(4))) float f32x4v;

// Built with the packed f32 VALU forms (v_pk_add / mul / fma_f32) off, as
// gemm_mxfp4_tile_kernel is; the helpers carry the attribute too so that
// they inline.  The host pass does not know the feature.
#if defined(__HIP_DEVICE_COMPILE__)
#define SGMV_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define SGMV_NO_PK_F32
#endif
#define SGMV_DEV __device__ SGMV_NO_PK_F32 __attribute__((always_inline)) inline

SGMV_DEV float sgmv_bf2f(unsigned short u) {
  union { uint32_t i; float f; } v;
  v.i = uint32_t(u) << 16;
  return v.f;
}

SGMV_DEV unsigned short sgmv_f2bf(float f) {  // round-to-nearest-even
  union { float f; uint32_t i; } v;
  v.f = f;
  return (unsigned short)((v.i + 0x7fffu + ((v.i >> 16) & 1u)) >> 16);
}

SGMV_DEV void sgmv_barrier() {  // __syncthreads() for such a kernel
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#endif
}

// Block-uniform: tile ti as (row0, nrows, a), false when it must be
// skipped.  The three words are read by every lane from one address.
SGMV_DEV bool sgmv_tile(const int* __restrict__ tiles, int ti, int T, int NA,
                        int& row0, int& nrows, int& a) {
  row0 = __builtin_amdgcn_readfirstlane(tiles[3 * ti]);
  nrows = __builtin_amdgcn_readfirstlane(tiles[3 * ti + 1]);
  a = __builtin_amdgcn_readfirstlane(tiles[3 * ti + 2]);
  return a >= 0 && a < NA && nrows >= 1 && nrows <= 16 && row0 >= 0 &&
         row0 <= T - nrows;
}

// ---------------------------------------------------------------------
// shrink.  One workgroup of SGMV_SHRINK_WAVES waves per tile.  The
// product runs transposed: the adapter's R rows are the MFMA's A operand
// (R / 16 fragments; R = 8 is one fragment with 8 live rows), the tile's
// x rows its B operand.  Both are K-contiguous, so a lane loads its 8 k
// of a row straight from global memory with one 16 B load, no LDS.  A
// lane then holds t[row0 + lq][16 f + 4 lh .. + 3]: one 16 B store.
//
// K is cut into 32-wide MFMA steps and every wave owns one contiguous,
// 32-aligned share of ceil(steps / waves) of them (the trailing waves own
// fewer or none).  Eight waves, not four: at K = 14336 that halves the
// serial chain of a wave to 56 steps and doubles the loads in flight per
// tile, which is what a table of few tiles is short of, and it needs no
// second launch and no f32 slabs as a gridDim.y split would.  The waves'
// partial accumulators meet in LDS and are added in the fixed order
// ((((0 + 1) + 2) + ...) + 7), the skinny_gemm_ws pattern.
// ---------------------------------------------------------------------
#define SGMV_SHRINK_WAVES 8
#define SGMV_SHRINK_THREADS (64 * SGMV_SHRINK_WAVES)

template <int R>
__global__ __launch_bounds__(SGMV_SHRINK_THREADS) SGMV_NO_PK_F32
void lora_sgmv_shrink_kernel(float* __restrict__ t,
                             const unsigned short* __restrict__ x,
                             const unsigned short* __restrict__ A,
                             const int* __restrict__ tiles, int T, int NA,
                             int K) {
  constexpr int NF = (R + 15) / 16;  // fragments of 16 adapter rows
  // part[wave][fragment][lane]: a lane's f32x4v, written and read as 16 B
  __shared__ f32x4v part[SGMV_SHRINK_WAVES][NF][64];
  int row0, nrows, a;
  if (!sgmv_tile(tiles, blockIdx.x, T, NA, row0, nrows, a)) return;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lq = lane & 15;
  const int lh = lane >> 4;
  const int steps = K >> 5;
  const int share = (steps + SGMV_SHRINK_WAVES - 1) / SGMV_SHRINK_WAVES;
  const int s0 = min(wave * share, steps);
  const int s1 = min(s0 + share, steps);

  const unsigned short* xp =
      x + (size_t)(row0 + min(lq, nrows - 1)) * K + lh * 8;
  const unsigned short* ap[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f)
    ap[f] = A + ((size_t)a * R + min(16 * f + lq, R - 1)) * K + lh * 8;

  f32x4v acc[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) acc[f] = f32x4v{0.f, 0.f, 0.f, 0.f};
  // four steps at a time, all their loads issued before the first MFMA;
  // the steps are still added in ascending order
  int s = s0;
  for (; s + 4 <= s1; s += 4) {
    short8v xf[4], af[4][NF];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      xf[u] = *reinterpret_cast<const short8v*>(xp + ((s + u) << 5));
#pragma unroll
      for (int f = 0; f < NF; ++f)
        af[u][f] =
            *reinterpret_cast<const short8v*>(ap[f] + ((s + u) << 5));
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int f = 0; f < NF; ++f)
        acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[u][f], xf[u],
                                                         acc[f], 0, 0, 0);
  }
  for (; s < s1; ++s) {
    const short8v xf = *reinterpret_cast<const short8v*>(xp + (s << 5));
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const short8v af = *reinterpret_cast<const short8v*>(ap[f] + (s << 5));
      acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, xf, acc[f], 0, 0,
                                                       0);
    }
  }
#pragma unroll
  for (int f = 0; f < NF; ++f) part[wave][f][lane] = acc[f];
  sgmv_barrier();

  // fold: thread (f, lane) of the first NF waves owns one f32x4v
  if (tid >= NF * 64) return;
  const int f = tid >> 6;
  f32x4v sum = part[0][f][lane];
#pragma unroll
  for (int w = 1; w < SGMV_SHRINK_WAVES; ++w) {
    const f32x4v p = part[w][f][lane];
#pragma unroll
    for (int r = 0; r < 4; ++r) sum[r] += p[r];
  }
  const int j = 16 * f + 4 * lh;  // R % 4 == 0: j < R means j + 3 < R
  if (lq < nrows && j < R)
    *reinterpret_cast<f32x4v*>(t + (size_t)(row0 + lq) * R + j) = sum;
}

void launch_lora_sgmv_shrink(void* t, const void* x, const void* A,
                             const void* tiles, int ntiles, int T, int NA,
                             int R, int K, void* stream) {
  if (ntiles <= 0 || T <= 0 || NA <= 0) return;
#define SGMV_SHRINK_CASE(RR)                                               \
  case RR:                                                                 \
    hipLaunchKernelGGL(lora_sgmv_shrink_kernel<RR>, dim3(ntiles),          \
                       dim3(SGMV_SHRINK_THREADS), 0, (hipStream_t)stream,  \
                       (float*)t, (const unsigned short*)x,                \
                       (const unsigned short*)A, (const int*)tiles, T, NA, \
                       K);                                                 \
    break;
  switch (R) {
    SGMV_SHRINK_CASE(8)
    SGMV_SHRINK_CASE(16)
    SGMV_SHRINK_CASE(32)
    SGMV_SHRINK_CASE(64)
    default: break;  // the binding rejects other ranks
  }
#undef SGMV_SHRINK_CASE
}

// ---------------------------------------------------------------------
// expand.  t is f32 and the fast MFMA takes bf16, so t is split in
// registers into hi = bf16(t) and lo = bf16(t - hi): t - hi is exact in
// f32 and |t - hi - lo| <= 2^-18 |t|.  Both halves go through the MFMA
// against the same Bm values.  The order of an MFMA's 32 k-slots is free
// as long as both operands agree, so one MFMA takes 16 ranks,
//   slots = hi[j0 .. j0 + 15] | lo[j0 .. j0 + 15]       (R >= 16)
//   slots = hi[0 .. 7] | lo[0 .. 7] | 0 | 0             (R == 8)
// and a 16 x 16 output fragment costs R / 16 MFMAs (one for R = 8).  The
// zero slots are zero on BOTH operands: 0 x NaN would reach live outputs.
//
// The product runs transposed, as in gemm_mxfp4_tile_kernel: Bm rows are
// the A operand and t rows the B operand, so a lane holds four
// consecutive n of one y row.  The accumulator is seeded with float(y)
// from one 8 B load, the MFMAs add the delta in f32, and the result is
// rounded once and stored with one 8 B store.
//
// Grid (ceil(N / 256), ceil(ntiles / 4)), four independent waves per
// workgroup (no LDS, no barrier).  A wave owns 64 columns (four
// fragments) and walks its workgroup's four consecutive tiles; its Bm
// fragments stay in registers while the adapter does not change.  (A
// wave's Bm fragments are 2 to 8 KiB against 4 KiB of y traffic per
// tile, so reloading them for every tile would cost as much as y.)
// ---------------------------------------------------------------------
#define SGMV_EXPAND_THREADS 256
#define SGMV_EXPAND_NI 4                       // 16-wide fragments per wave
#define SGMV_EXPAND_BN (4 * 16 * SGMV_EXPAND_NI)  // n per workgroup
#define SGMV_EXPAND_TPB 4                      // tiles per workgroup

// the 8 bf16 k-slots of t[j .. j + 7]: hi halves, or lo halves
template <bool LO>
SGMV_DEV short8v sgmv_split8(const float* __restrict__ tp) {
  const f32x4v u0 = *reinterpret_cast<const f32x4v*>(tp);
  const f32x4v u1 = *reinterpret_cast<const f32x4v*>(tp + 4);
  short8v out;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float v = i < 4 ? u0[i] : u1[i - 4];
    const unsigned short hi = sgmv_f2bf(v);
    out[i] = (short)(LO ? sgmv_f2bf(v - sgmv_bf2f(hi)) : hi);
  }
  return out;
}

template <int R>
__global__ __launch_bounds__(SGMV_EXPAND_THREADS) SGMV_NO_PK_F32
void lora_sgmv_expand_kernel(unsigned short* __restrict__ y,
                             const float* __restrict__ t,
                             const unsigned short* __restrict__ Bm,
                             const int* __restrict__ tiles, int ntiles,
                             int T, int NA, int N) {
  constexpr int NM = (R + 15) / 16;  // MFMAs per output fragment
  constexpr int NI = SGMV_EXPAND_NI;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lq = lane & 15;
  const int lh = lane >> 4;
  const int wn0 = blockIdx.x * SGMV_EXPAND_BN + wave * (16 * NI);
  if (wn0 >= N) return;  // wave-uniform; nothing below synchronises
  // this lane's k-slot chunk lh of MFMA m: ranks jof + 16 m .. + 7, hi or
  // lo half; R == 8 has two live chunks
  const bool live_k = R >= 16 || lh < 2;
  const bool lo = R >= 16 ? lh >= 2 : lh == 1;
  const int jof = R >= 16 ? (lh & 1) * 8 : 0;
  const short8v zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

  short8v bf[NI][NM];
  int cur = -1;  // adapter whose fragments bf holds
  const int t_end = min(ntiles, (int)(blockIdx.y + 1) * SGMV_EXPAND_TPB);
  for (int ti = blockIdx.y * SGMV_EXPAND_TPB; ti < t_end; ++ti) {
    int row0, nrows, a;
    if (!sgmv_tile(tiles, ti, T, NA, row0, nrows, a)) continue;
    if (a != cur) {
      cur = a;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int n = min(wn0 + 16 * i + lq, N - 1);
        const unsigned short* bp = Bm + ((size_t)a * N + n) * R + jof;
#pragma unroll
        for (int m = 0; m < NM; ++m)
          bf[i][m] = live_k
                         ? *reinterpret_cast<const short8v*>(bp + 16 * m)
                         : zero8;
      }
    }
    const int row = row0 + min(lq, nrows - 1);
    const float* tp = t + (size_t)row * R + jof;
    short8v tf[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m)
      tf[m] = !live_k ? zero8
              : lo    ? sgmv_split8<true>(tp + 16 * m)
                      : sgmv_split8<false>(tp + 16 * m);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      if (wn0 + 16 * i >= N) break;  // wave-uniform
      const int n = wn0 + 16 * i + 4 * lh;  // N % 8 == 0: n < N, n + 3 < N
      const bool live = lq < nrows && n < N;
      unsigned short* yp = y + (size_t)row * N + n;
      ushort4 v = {0, 0, 0, 0};
      if (live) v = *reinterpret_cast<const ushort4*>(yp);
      f32x4v acc = {sgmv_bf2f(v.x), sgmv_bf2f(v.y), sgmv_bf2f(v.z),
                    sgmv_bf2f(v.w)};
#pragma unroll
      for (int m = 0; m < NM; ++m)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[i][m], tf[m], acc, 0,
                                                      0, 0);
      if (live) {
        v.x = sgmv_f2bf(acc[0]);
        v.y = sgmv_f2bf(acc[1]);
        v.z = sgmv_f2bf(acc[2]);
        v.w = sgmv_f2bf(acc[3]);
        *reinterpret_cast<ushort4*>(yp) = v;
      }
    }
  }
}

void launch_lora_sgmv_expand(void* y, const void* t, const void* Bm,
                             const void* tiles, int ntiles, int T, int NA,
                             int R, int N, void* stream) {
  if (ntiles <= 0 || T <= 0 || NA <= 0 || N <= 0) return;
  const dim3 grid((N + SGMV_EXPAND_BN - 1) / SGMV_EXPAND_BN,
                  (ntiles + SGMV_EXPAND_TPB - 1) / SGMV_EXPAND_TPB);
#define SGMV_EXPAND_CASE(RR)                                               \
  case RR:                                                                 \
    hipLaunchKernelGGL(lora_sgmv_expand_kernel<RR>, grid,                  \
                       dim3(SGMV_EXPAND_THREADS), 0, (hipStream_t)stream,  \
                       (unsigned short*)y, (const float*)t,                \
                       (const unsigned short*)Bm, (const int*)tiles,       \
                       ntiles, T, NA, N);                             \
    break;
  switch (R) {
    SGMV_EXPAND_CASE(8)
    SGMV_EXPAND_CASE(16)
    SGMV_EXPAND_CASE(32)
    SGMV_EXPAND_CASE(64)
    default: break;  // the binding rejects other ranks
  }
#undef SGMV_EXPAND_CASE
}
