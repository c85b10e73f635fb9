// Copyright 2026 mlrun_amd authors
//
// Licensed under the Apache License, Version 2.0 (the "License");
// you may not use this file except in compliance with the License.
//
// PROMPT SCORING for gfx950: for every row t of h [T, K] and its target
// token, the target's logit and the log-sum-exp of the row's V logits
//   z[t, v]  = bf16(h[t, :] . w[v, :])         (never stored)
//   z_tgt[t] = z[t, targets[t]]                 (0 when out of [0, V))
//   lse[t]   = log sum_v exp(z[t, v])
//   logprob[t] = z_tgt[t] - lse[t]
// without a [T, V] buffer of any dtype: a vocabulary-wide GEMM whose
// epilogue is a log-sum-exp and a gather, the logits living in the
// accumulator registers only.
//
// Logits contract.  z[t, v] is bit for bit what gemm_bf16_tile_kernel
// stores for that row and column: the K loop IS that kernel's
// (bf16_tile_kloop.inc: LDS-DMA of both operands, two stages, one barrier
// per stage, XOR-permuted 128 B rows, the K % 64 == 32 tail, clamped rows),
// one accumulator per logit, 32-k blocks in ascending k, one
// v_mfma_f32_16x16x32_bf16 each, then the same f2bf.  Scoring and
// generation see one model.
//
// Decomposition.  One workgroup per 128 x BN tile of the logits, 4 waves
// 2 x 2, a wave owns 64 rows x BN/2 columns (gemm_bf16_tile.hip).  After
// the K loop lane (lq, lh) holds, for each of its four rows m = wm0 + 16 j
// + lq, the 4 consecutive columns wn0 + 16 i + 4 lh .. of BN/32
// accumulators.  Epilogue of a wave, per row:
//   round to bf16 and widen; columns >= V (clamped loads, copies of row
//   V - 1) become -inf first;
//   the lane that holds column targets[m] stores it to z_tgt[m] (one
//   owner in the whole grid, or none);
//   register max, then xor 16 / xor 32 across the four lh groups;
//   sum of expf(z - max) in registers, in ascending column order, then
//   the same two cross-lane steps: the wave partial (m, l), l = sum
//   exp(z - m), natural domain, identical in the four lane groups.
// The two waves of a row range are then combined in the workgroup: the
// right-hand wave leaves its 64 partials in LDS (the stage buffers are
// dead after one more barrier), the left-hand one folds them in,
//   M = max(m0, m1),  l = l0 exp(m0 - M) + l1 exp(m1 - M),
// and stores (M, l) to ws[m, tile column] with a plain 8 B store.  So P =
// ceil(V / BN) partials per row, no atomics.  A right-hand wave that lies
// wholly outside V contributes the neutral (-1e30, 0); -inf is never a
// maximum that is subtracted (a wave's maximum is clamped to -1e30, and
// exp(-inf - m) is 0).  Rows >= T are never stored.
//
// lm_head_logprobs_fold_kernel: one wave per row.  Lane q takes partials
// q, q + 64, ..: the row maximum first (exact), then sum l_p exp(m_p - M)
// in ascending p, then a xor butterfly 1, 2, .. 32.  The order depends on
// P = ceil(V / BN) alone.  It writes lse = M + logf(l), z_tgt = 0 for a
// target outside [0, V), and logprob = z_tgt - lse.
//
// Grid order.  The grid is one-dimensional and M TILES RUN FASTEST: the
// ceil(T / 128) workgroups that read one BN-row slice of the 128256-row
// weight are neighbours in launch order, so the slice is fetched from HBM
// once and found in L2 by the others, while the whole activation (T x K,
// 16 MB at T 2048) stays resident.  The other order (column tiles fastest,
// the sibling GEMM's) is kept behind `order` = 1 of the launcher for
// measuring one against the other; docs/kernels.md has the numbers.
//
// expf / logf are the accurate library functions (1 ulp each).  The
// epilogue is fp32 VALU code after the loop, ~6 instructions per logit
// against 2 K / 32 MFMA-issues per 4 logits; the kernel does not carry the
// no-packed-fp32-ops attribute of the fp8 and mxfp4 tile kernels, so every
// helper and the .inc's lambda inline as plain always_inline code
// (docs/kernels.md: private segment 0, no call instruction).
//
// Capture-safe: no allocation, no sync, no memset.

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "bf16_tile_loop.h"
#include "kernels.h"

#define LHL_NEUTRAL (-1e30f)  // maximum of a partial without columns

B16T_DEV float lhl_bf2f(unsigned short b) {
  union { uint32_t i; float f; } v;
  v.i = (uint32_t)b << 16;
  return v.f;
}

// (m, l) + (m2, l2) in the order written
B16T_DEV float2 lhl_combine(float2 a, float2 b) {
  const float mx = fmaxf(a.x, b.x);
  return make_float2(mx, a.y * expf(a.x - mx) + b.y * expf(b.x - mx));
}

template <int BN>
__global__ __launch_bounds__(256) void lm_head_logprobs_kernel(
    float* __restrict__ z_tgt, float2* __restrict__ ws,
    const unsigned char* __restrict__ A,  // h [M = T, K] bf16
    const unsigned char* __restrict__ W,  // w [N = V, K] bf16
    const int* __restrict__ targets, int M, int N, int K, int mtiles,
    int ntiles, int order) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lq = lane & 15;
  const int lh = lane >> 4;
  const int bid = blockIdx.x;
  const int mt = order == 0 ? bid % mtiles : bid / ntiles;
  const int nt = order == 0 ? bid / mtiles : bid % ntiles;
  const int m0 = mt * B16T_BM;
  const int n0 = nt * BN;
  const int wm0 = m0 + (wave >> 1) * 64;  // this wave's sub-tile
  const int wn0 = n0 + (wave & 1) * (BN / 2);
  const bool active = wm0 < M && wn0 < N;  // wave-uniform
#include "bf16_tile_kloop.inc"  // the K loop: declares lds and acc

  // --- wave partials: part[j] = (max, sum exp) of row wm0 + 16 j + lq over
  // this wave's columns < N
  float2 part[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    part[j] = make_float2(LHL_NEUTRAL, 0.f);
    if (!active) continue;
    const int m = wm0 + 16 * j + lq;
    const int tgt = m < M ? targets[m] : -1;
    float z[NI][4];
    float mx = -INFINITY, zt = 0.f;
    bool owner = false;  // tgt >= 0 only where m < M
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = wn0 + 16 * i + 4 * lh + r;
        const float v =
            n < N ? lhl_bf2f(b16t_f2bf(acc[j][i][r])) : -INFINITY;
        if (n < N && n == tgt) { owner = true; zt = v; }
        z[i][r] = v;
        mx = fmaxf(mx, v);
      }
    if (owner) z_tgt[m] = zt;
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    mx = fmaxf(mx, LHL_NEUTRAL);
    float l = 0.f;
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) l += expf(z[i][r] - mx);
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    part[j] = make_float2(mx, l);
  }

  // --- the right-hand wave of a row range hands its partials over in LDS
  float2* xch = reinterpret_cast<float2*>(lds);  // [2 row halves][64 rows]
  b16t_barrier();  // every wave is done with the last stage
  if ((wave & 1) && lh == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      xch[(wave >> 1) * 64 + 16 * j + lq] = part[j];
  }
  b16t_barrier();
  if ((wave & 1) || lh != 0) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int m = wm0 + 16 * j + lq;
    if (m >= M) continue;
    ws[(size_t)m * ntiles + nt] =
        lhl_combine(part[j], xch[(wave >> 1) * 64 + 16 * j + lq]);
  }
}

// One wave per row, 4 rows per workgroup.
__global__ __launch_bounds__(256) void lm_head_logprobs_fold_kernel(
    float* __restrict__ logprob, float* __restrict__ lse,
    float* __restrict__ z_tgt, const float2* __restrict__ ws,
    const int* __restrict__ targets, int T, int V, int P) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= T) return;  // wave-uniform; no barrier below
  const float2* p = ws + (size_t)row * P;
  float mx = LHL_NEUTRAL;
  for (int q = lane; q < P; q += 64) mx = fmaxf(mx, p[q].x);
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) mx = fmaxf(mx, __shfl_xor(mx, s));
  float l = 0.f;
  for (int q = lane; q < P; q += 64) {
    const float2 v = p[q];
    l += v.y * expf(v.x - mx);
  }
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) l += __shfl_xor(l, s);
  if (lane != 0) return;
  const float r = mx + logf(l);
  const int tgt = targets[row];
  float z = 0.f;
  if (tgt >= 0 && tgt < V) z = z_tgt[row];
  else z_tgt[row] = 0.f;
  lse[row] = r;
  logprob[row] = z - r;
}

// partials per row at tile width bn
static int lhl_ntiles(int V, int bn) { return (V + bn - 1) / bn; }

// float2 elements of a workspace that serves every tile width
long long lm_head_logprobs_ws_pairs(int T, int V) {
  return (long long)T * lhl_ntiles(V, 64);
}

// bn: 128 or 64 forces the tile width, 0 picks it (the rule and what it
// was measured on: docs/kernels.md).  order 0: M tiles fastest (the
// default), 1: column tiles fastest.
void launch_lm_head_logprobs(void* logprob, void* lse, void* z_tgt, void* ws,
                             const void* h, const void* w,
                             const void* targets, int T, int V, int K, int bn,
                             int order, void* stream) {
  const int mtiles = (T + B16T_BM - 1) / B16T_BM;
  if (bn == 0) bn = (long long)mtiles * ((V + 63) / 64) <= 512 ? 64 : 128;
  const int ntiles = lhl_ntiles(V, bn);
  auto kern = bn == 64 ? lm_head_logprobs_kernel<64>
                       : lm_head_logprobs_kernel<128>;
  hipLaunchKernelGGL(kern, dim3((unsigned)(mtiles * ntiles)), dim3(256), 0,
                     (hipStream_t)stream, (float*)z_tgt, (float2*)ws,
                     (const unsigned char*)h, (const unsigned char*)w,
                     (const int*)targets, T, V, K, mtiles, ntiles, order);
  hipLaunchKernelGGL(lm_head_logprobs_fold_kernel, dim3((T + 3) / 4),
                     dim3(256), 0, (hipStream_t)stream, (float*)logprob,
                     (float*)lse, (float*)z_tgt, (const float2*)ws,
                     (const int*)targets, T, V, ntiles);
}
