// Copyright 2026 mlrun_amd authors
//
// Licensed under the Apache License, Version 2.0 (the "License");
// you may not use this file except in compliance with the License.
//
// The K loop of the bf16 output-tile kernels (see gemm_bf16_tile.hip for
// the design), included INSIDE a kernel body templated on BN.  It is text
// and not a function because gemm_bf16_tile_kernel's code object must stay
// what it was: as a function taking the accumulators by reference the same
// statements compiled to twice the accumulator registers.
//
// Expects in scope: A, W (const unsigned char*), M, N, K, lane, wave, lq,
// lh, m0, n0 and the wave-uniform `active`.  Declares the two LDS stages
// `lds` and leaves
//   acc[j][i][r] = sum_k A[wm0 + 16 j + lq][k] W[wn0 + 16 i + 4 lh + r][k]
// with wm0 = m0 + (wave >> 1) * 64, wn0 = n0 + (wave & 1) * (BN / 2); rows
// >= M and >= N repeat the last row; acc stays zero in a wave that is not
// active.  Other waves may still read the last stage's buffer at the end.

  constexpr int NI = BN / 32;              // 16-wide n sub-tiles of a wave
  constexpr int A_B = B16T_BM * B16T_ROW;  // bytes of the A tile of a stage
  constexpr int STAGE_B = A_B + BN * B16T_ROW;
  constexpr int NDMA_A = B16T_BM / 32;     // DMA instructions of a wave
  constexpr int NDMA_W = BN / 32;
  __shared__ __attribute__((aligned(1024))) unsigned char lds[2 * STAGE_B];
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
