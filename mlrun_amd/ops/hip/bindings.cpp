// Copyright 2026 mlrun_amd authors
//
// Licensed under the Apache License, Version 2.0 (the "License");
// you may not use this file except in compliance with the License.
//
// Torch bindings for the CDNA4 kernel library (mlrun_amd._hip_ops).
// Thin validation + launch layer; kernels live in kernels.hip.

#include <climits>

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "kernels.h"

#define CHECK_DEV(x) TORCH_CHECK((x).is_cuda(), #x " must be on GPU")
#define CHECK_CONTIG(x) TORCH_CHECK((x).is_contiguous(), #x " not contiguous")
#define CHECK_BF16(x) \
  TORCH_CHECK((x).scalar_type() == torch::kBFloat16, #x " must be bf16")
#define CHECK_F32(x) \
  TORCH_CHECK((x).scalar_type() == torch::kFloat32, #x " must be f32")

#define CHECK_U8(x) \
  TORCH_CHECK((x).scalar_type() == torch::kUInt8, #x " must be uint8")

#define CHECK_I32(x) \
  TORCH_CHECK((x).scalar_type() == torch::kInt32, #x " must be int32")

// native ROCm stream accessor (c10::hip — no hipify pass needed; the
// kernels in kernels.hip are pure CDNA4 HIP already)
static void* stream() {
  return (void*)c10::hip::getCurrentHIPStream().stream();
}

// out <- rmsnorm(x [+ residual]); residual updated in-place when given
void fused_add_rmsnorm(torch::Tensor out, torch::Tensor x,
                       torch::Tensor weight,
                       c10::optional<torch::Tensor> residual, double eps,
                       c10::optional<torch::Tensor> out8,
                       c10::optional<torch::Tensor> out_scale) {
  CHECK_DEV(out); CHECK_CONTIG(out); CHECK_BF16(out);
  CHECK_DEV(x); CHECK_CONTIG(x); CHECK_BF16(x);
  CHECK_DEV(weight); CHECK_CONTIG(weight); CHECK_BF16(weight);
  int64_t hidden = x.size(-1);
  int64_t rows = x.numel() / hidden;
  TORCH_CHECK(hidden % 8 == 0, "hidden must be a multiple of 8");
  TORCH_CHECK(weight.numel() == hidden, "weight size mismatch");
  void* res_ptr = nullptr;
  if (residual.has_value()) {
    CHECK_DEV(*residual); CHECK_CONTIG(*residual); CHECK_BF16(*residual);
    TORCH_CHECK(residual->numel() == x.numel(), "residual size mismatch");
    res_ptr = residual->data_ptr();
  }
  void* out8_ptr = nullptr;
  void* scale_ptr = nullptr;
  if (out8.has_value()) {
    TORCH_CHECK(out_scale.has_value(), "out8 needs out_scale");
    TORCH_CHECK(out8->numel() == x.numel() &&
                out_scale->numel() >= rows, "fp8 sidecar sizes");
    TORCH_CHECK(hidden % 64 == 0, "fp8 sidecar needs hidden % 64 == 0");
    out8_ptr = out8->data_ptr();
    scale_ptr = out_scale->data_ptr();
  }
  launch_fused_add_rmsnorm(out.data_ptr(), res_ptr, x.data_ptr(),
                           weight.data_ptr(), (int)rows, (int)hidden,
                           (float)eps, out8_ptr, scale_ptr, stream());
}

// q may be a strided row-view into a fused qkv buffer:
// required layout [T, heads, dim] with strides (row_stride, dim, 1)
static long long check_head_view(const torch::Tensor& q) {
  TORCH_CHECK(q.dim() == 3, "expected [T, heads, dim]");
  TORCH_CHECK(q.stride(2) == 1 && q.stride(1) == q.size(2),
              "inner dims must be dense (strides (*, dim, 1))");
  return (long long)q.stride(0);
}

void rope(torch::Tensor q, torch::Tensor positions, torch::Tensor cos_sin) {
  CHECK_DEV(q); CHECK_BF16(q);
  CHECK_DEV(positions); CHECK_CONTIG(positions); CHECK_I32(positions);
  CHECK_DEV(cos_sin); CHECK_CONTIG(cos_sin); CHECK_F32(cos_sin);
  long long row_stride = check_head_view(q);
  int T = q.size(0), heads = q.size(1), dim = q.size(2);
  TORCH_CHECK(dim % 2 == 0 && dim / 2 <= 1024, "bad head dim");
  TORCH_CHECK(positions.numel() == T, "positions size mismatch");
  launch_rope(q.data_ptr(), positions.data_ptr(), cos_sin.data_ptr(), T,
              heads, dim, row_stride, stream());
}

void swiglu_fused(torch::Tensor out, torch::Tensor gu) {
  CHECK_DEV(out); CHECK_CONTIG(out); CHECK_BF16(out);
  CHECK_DEV(gu); CHECK_CONTIG(gu); CHECK_BF16(gu);
  TORCH_CHECK(gu.dim() == 2 && out.dim() == 2, "need 2-D tensors");
  int rows = gu.size(0), inter = gu.size(1) / 2;
  TORCH_CHECK(out.size(0) == rows && out.size(1) == inter, "shape mismatch");
  TORCH_CHECK(inter % 8 == 0, "inter must be a multiple of 8");
  launch_swiglu_fused(out.data_ptr(), gu.data_ptr(), rows, inter, stream());
}

void silu_mul(torch::Tensor out, torch::Tensor gate, torch::Tensor up) {
  CHECK_DEV(out); CHECK_CONTIG(out); CHECK_BF16(out);
  CHECK_DEV(gate); CHECK_CONTIG(gate); CHECK_BF16(gate);
  CHECK_DEV(up); CHECK_CONTIG(up); CHECK_BF16(up);
  TORCH_CHECK(out.numel() == gate.numel() && gate.numel() == up.numel(),
              "size mismatch");
  TORCH_CHECK(out.numel() % 8 == 0, "numel must be a multiple of 8");
  launch_silu_mul(out.data_ptr(), gate.data_ptr(), up.data_ptr(),
                  out.numel(), stream());
}

// out_bf16 [M,N] <- A [M,K] @ W [N,K]^T.  part_f32 is the split-K
// scratch ([ksplit*M*N] f32, unused when ksplit==1 — pass any tensor).
void skinny_gemm(torch::Tensor out_bf16, torch::Tensor part_f32,
                 torch::Tensor a, torch::Tensor w, int64_t ksplit,
                 int64_t variant) {
  CHECK_DEV(out_bf16); CHECK_CONTIG(out_bf16); CHECK_BF16(out_bf16);
  CHECK_DEV(a); CHECK_CONTIG(a); CHECK_BF16(a);
  CHECK_DEV(w); CHECK_CONTIG(w); CHECK_BF16(w);
  int M = a.size(0), K = a.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K, "K mismatch");
  TORCH_CHECK(M <= 64, "skinny_gemm supports M <= 64");
  TORCH_CHECK(K % 32 == 0, "K must be a multiple of 32");
  TORCH_CHECK(out_bf16.numel() == (int64_t)M * N, "out shape mismatch");
  if (ksplit > 1) {
    CHECK_DEV(part_f32); CHECK_CONTIG(part_f32); CHECK_F32(part_f32);
    TORCH_CHECK(part_f32.numel() >= ksplit * (int64_t)M * N,
                "part_f32 scratch too small");
  }
  launch_skinny_gemm(out_bf16.data_ptr(),
                     ksplit > 1 ? part_f32.data_ptr() : nullptr,
                     a.data_ptr(), w.data_ptr(), M, N, K, (int)ksplit,
                     (int)variant, stream());
}

void skinny_gemm_slabs(torch::Tensor part_f32, torch::Tensor a,
                       torch::Tensor w, int64_t ksplit, int64_t variant) {
  CHECK_DEV(part_f32); CHECK_CONTIG(part_f32); CHECK_F32(part_f32);
  CHECK_DEV(a); CHECK_CONTIG(a); CHECK_BF16(a);
  CHECK_DEV(w); CHECK_CONTIG(w); CHECK_BF16(w);
  int M = a.size(0), K = a.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K && M <= 64 && K % 32 == 0, "bad shapes");
  TORCH_CHECK(part_f32.numel() >= ksplit * (int64_t)M * N,
              "part_f32 scratch too small");
  launch_skinny_gemm_slabs(part_f32.data_ptr(), a.data_ptr(), w.data_ptr(),
                           M, N, K, (int)ksplit, (int)variant, stream());
}

void fused_add_rmsnorm_slab(torch::Tensor out, torch::Tensor residual,
                            torch::Tensor slabs, torch::Tensor weight,
                            int64_t ksplit, double eps) {
  CHECK_DEV(out); CHECK_CONTIG(out); CHECK_BF16(out);
  CHECK_DEV(residual); CHECK_CONTIG(residual); CHECK_BF16(residual);
  CHECK_DEV(slabs); CHECK_CONTIG(slabs); CHECK_F32(slabs);
  CHECK_DEV(weight); CHECK_CONTIG(weight); CHECK_BF16(weight);
  int64_t hidden = out.size(-1);
  int64_t rows = out.numel() / hidden;
  TORCH_CHECK(hidden % 8 == 0, "hidden must be a multiple of 8");
  TORCH_CHECK(ksplit >= 1, "ksplit must be at least 1");
  TORCH_CHECK(residual.numel() == out.numel(), "residual size mismatch");
  TORCH_CHECK(weight.numel() == hidden, "weight size mismatch");
  TORCH_CHECK(slabs.numel() >= ksplit * rows * hidden, "slabs too small");
  launch_fused_add_rmsnorm_slab(out.data_ptr(), residual.data_ptr(),
                                slabs.data_ptr(), weight.data_ptr(),
                                (int)rows, (int)hidden, (float)eps,
                                (int)ksplit, stream());
}

void swiglu_slab(torch::Tensor out, torch::Tensor slabs, int64_t ksplit) {
  CHECK_DEV(out); CHECK_CONTIG(out); CHECK_BF16(out);
  CHECK_DEV(slabs); CHECK_CONTIG(slabs); CHECK_F32(slabs);
  TORCH_CHECK(out.dim() == 2, "out must be [rows, inter]");
  TORCH_CHECK(ksplit >= 1, "ksplit must be at least 1");
  int rows = out.size(0), inter = out.size(1);
  TORCH_CHECK(inter % 4 == 0, "inter must be a multiple of 4");
  TORCH_CHECK(slabs.numel() >= (int64_t)ksplit * rows * 2 * inter,
              "slabs too small");
  launch_swiglu_slab(out.data_ptr(), slabs.data_ptr(), rows, inter,
                     (int)ksplit, stream());
}

void rope_kv_slab(torch::Tensor qkv, torch::Tensor kc, torch::Tensor vc,
                  torch::Tensor slabs, torch::Tensor positions,
                  torch::Tensor cos_sin, int64_t hq, int64_t ksplit) {
  CHECK_DEV(qkv); CHECK_CONTIG(qkv); CHECK_BF16(qkv);
  CHECK_DEV(kc); CHECK_CONTIG(kc); CHECK_BF16(kc);
  CHECK_DEV(vc); CHECK_CONTIG(vc); CHECK_BF16(vc);
  CHECK_DEV(slabs); CHECK_CONTIG(slabs); CHECK_F32(slabs);
  CHECK_DEV(positions); CHECK_CONTIG(positions); CHECK_I32(positions);
  CHECK_DEV(cos_sin); CHECK_CONTIG(cos_sin); CHECK_F32(cos_sin);
  TORCH_CHECK(kc.dim() == 4 && vc.sizes() == kc.sizes(),
              "caches must be [B, Hkv, Smax, D] of equal shape");
  int B = kc.size(0), Hkv = kc.size(1), Smax = kc.size(2), D = kc.size(3);
  TORCH_CHECK(qkv.dim() == 2, "qkv must be [B, rows]");
  int qkv_row = qkv.size(1);
  TORCH_CHECK(hq >= 1 && qkv.size(0) == B &&
              qkv_row >= (hq + 2 * Hkv) * D, "qkv buffer too small");
  TORCH_CHECK(D % 2 == 0 && D / 2 <= 1024, "bad head dim");
  TORCH_CHECK(positions.numel() == B, "positions size mismatch");
  TORCH_CHECK(cos_sin.dim() == 3 && cos_sin.size(1) == D / 2 &&
              cos_sin.size(2) == 2, "cos_sin must be [max_pos, D/2, 2]");
  TORCH_CHECK(ksplit >= 1, "ksplit must be at least 1");
  TORCH_CHECK(slabs.numel() >= (int64_t)ksplit * B * qkv_row,
              "slabs too small");
  launch_rope_kv_slab(qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                      slabs.data_ptr(), positions.data_ptr(),
                      cos_sin.data_ptr(), B, (int)hq, Hkv, Smax, D, qkv_row,
                      (int)ksplit, stream());
}

void rope_kv_fused(torch::Tensor qkv, torch::Tensor kc, torch::Tensor vc,
                   torch::Tensor positions, torch::Tensor cos_sin,
                   int64_t hq,
                   c10::optional<torch::Tensor> k_scale = c10::nullopt,
                   c10::optional<torch::Tensor> v_scale = c10::nullopt) {
  CHECK_DEV(qkv); CHECK_CONTIG(qkv); CHECK_BF16(qkv);
  CHECK_DEV(kc); CHECK_CONTIG(kc);
  CHECK_DEV(vc); CHECK_CONTIG(vc);
  CHECK_DEV(positions); CHECK_CONTIG(positions); CHECK_I32(positions);
  CHECK_DEV(cos_sin); CHECK_CONTIG(cos_sin); CHECK_F32(cos_sin);
  int B = kc.size(0), Hkv = kc.size(1), Smax = kc.size(2), D = kc.size(3);
  TORCH_CHECK(qkv.dim() == 2 && qkv.size(0) == B, "qkv must be [B, rows]");
  TORCH_CHECK(qkv.size(1) >= (hq + 2 * Hkv) * D, "qkv row too small");
  if (k_scale.has_value()) {
    // fp8 KV mode: caches are uint8 e4m3 + per-row f32 scales
    TORCH_CHECK(v_scale.has_value(), "fp8 KV needs both scales");
    CHECK_U8(kc); CHECK_U8(vc);
    CHECK_DEV(*k_scale); CHECK_CONTIG(*k_scale); CHECK_F32(*k_scale);
    CHECK_DEV(*v_scale); CHECK_CONTIG(*v_scale); CHECK_F32(*v_scale);
    TORCH_CHECK(k_scale->numel() >= (int64_t)B * Hkv * Smax &&
                v_scale->numel() >= (int64_t)B * Hkv * Smax,
                "scale tensors too small");
    TORCH_CHECK(D == 128, "fp8 KV requires head_dim 128");
    launch_rope_kv_fused_q8(qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                            k_scale->data_ptr(), v_scale->data_ptr(),
                            positions.data_ptr(), cos_sin.data_ptr(), B,
                            (int)hq, Hkv, Smax, D, qkv.size(1), stream());
    return;
  }
  CHECK_BF16(kc); CHECK_BF16(vc);
  launch_rope_kv_fused(qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                       positions.data_ptr(), cos_sin.data_ptr(), B, (int)hq,
                       Hkv, Smax, D, qkv.size(1), stream());
}

void skinny_gemm_fp8(torch::Tensor out_bf16, torch::Tensor part_f32,
                     torch::Tensor a8, torch::Tensor a_scale,
                     torch::Tensor w8, torch::Tensor w_scale,
                     int64_t ksplit) {
  CHECK_DEV(out_bf16); CHECK_CONTIG(out_bf16); CHECK_BF16(out_bf16);
  CHECK_DEV(a8); CHECK_CONTIG(a8); CHECK_U8(a8);
  CHECK_DEV(w8); CHECK_CONTIG(w8); CHECK_U8(w8);
  CHECK_DEV(a_scale); CHECK_F32(a_scale);
  CHECK_DEV(w_scale); CHECK_F32(w_scale);
  int M = a8.size(0), K = a8.size(1), N = w8.size(0);
  TORCH_CHECK(w8.size(1) == K && M <= 64 && K % 64 == 0,
              "bad shapes (fp8 path needs K % 64 == 0)");
  TORCH_CHECK(a_scale.numel() >= M && w_scale.numel() >= N,
              "scale sizes");
  if (ksplit > 1) {
    CHECK_DEV(part_f32); CHECK_CONTIG(part_f32); CHECK_F32(part_f32);
    TORCH_CHECK(part_f32.numel() >= ksplit * (int64_t)M * N,
                "part_f32 scratch too small");
  }
  launch_skinny_gemm_fp8(out_bf16.data_ptr(),
                         ksplit > 1 ? part_f32.data_ptr() : nullptr,
                         a8.data_ptr(), a_scale.data_ptr(), w8.data_ptr(),
                         w_scale.data_ptr(), M, N, K, (int)ksplit,
                         stream());
}

void quant_fp8_rows(torch::Tensor a8, torch::Tensor a_scale,
                    torch::Tensor a) {
  CHECK_DEV(a8); CHECK_CONTIG(a8); CHECK_U8(a8);
  CHECK_DEV(a_scale); CHECK_F32(a_scale);
  CHECK_DEV(a); CHECK_CONTIG(a); CHECK_BF16(a);
  int64_t cols = a.size(-1);
  int64_t rows = a.numel() / cols;
  TORCH_CHECK(cols % 8 == 0, "cols must be a multiple of 8");
  TORCH_CHECK(a8.numel() == a.numel() && a_scale.numel() >= rows,
              "size mismatch");
  launch_quant_fp8_rows(a8.data_ptr(), a_scale.data_ptr(), a.data_ptr(),
                        (int)rows, (int)cols, stream());
}

void cast_f32_bf16(torch::Tensor out, torch::Tensor in) {
  CHECK_DEV(out); CHECK_CONTIG(out); CHECK_BF16(out);
  CHECK_DEV(in); CHECK_CONTIG(in); CHECK_F32(in);
  TORCH_CHECK(out.numel() == in.numel(), "size mismatch");
  launch_cast_f32_bf16(out.data_ptr(), in.data_ptr(), in.numel(), stream());
}

void attn_decode(torch::Tensor o, torch::Tensor q, torch::Tensor kc,
                 torch::Tensor vc, torch::Tensor seq_lens, double scale,
                 c10::optional<torch::Tensor> partial_ws, int64_t nsplit,
                 c10::optional<torch::Tensor> k_scale = c10::nullopt,
                 c10::optional<torch::Tensor> v_scale = c10::nullopt) {
  CHECK_DEV(o); CHECK_CONTIG(o); CHECK_BF16(o);
  CHECK_DEV(q); CHECK_BF16(q);
  CHECK_DEV(kc); CHECK_CONTIG(kc);
  CHECK_DEV(vc); CHECK_CONTIG(vc);
  const bool kvq = k_scale.has_value();
  if (kvq) {
    TORCH_CHECK(v_scale.has_value(), "fp8 KV needs both scales");
    CHECK_U8(kc); CHECK_U8(vc);
    CHECK_DEV(*k_scale); CHECK_CONTIG(*k_scale); CHECK_F32(*k_scale);
    CHECK_DEV(*v_scale); CHECK_CONTIG(*v_scale); CHECK_F32(*v_scale);
  } else {
    CHECK_BF16(kc); CHECK_BF16(vc);
  }
  CHECK_DEV(seq_lens); CHECK_CONTIG(seq_lens); CHECK_I32(seq_lens);
  TORCH_CHECK(q.dim() == 3 && kc.dim() == 4, "q [B,Hq,D], kc [B,Hkv,S,D]");
  long long q_row_stride = check_head_view(q);
  int B = q.size(0), Hq = q.size(1), D = q.size(2);
  int Hkv = kc.size(1), Smax = kc.size(2);
  TORCH_CHECK(D == 128, "attn_decode requires head_dim 128");
  TORCH_CHECK(Hq % Hkv == 0 && Hq / Hkv <= 8,
              "grouped heads per kv head must divide and be <= 8");
  TORCH_CHECK(kc.size(0) == B && kc.size(3) == D, "kc shape mismatch");
  TORCH_CHECK(vc.sizes() == kc.sizes(), "vc shape must equal kc shape");
  TORCH_CHECK(seq_lens.numel() == B, "seq_lens must hold B entries");
  TORCH_CHECK(nsplit >= 1 && nsplit <= 1024, "bad nsplit");
  float* ws = nullptr;
  if (nsplit > 1) {
    TORCH_CHECK(partial_ws.has_value(), "nsplit>1 needs partial_ws");
    CHECK_DEV(*partial_ws); CHECK_CONTIG(*partial_ws);
    CHECK_F32(*partial_ws);
    TORCH_CHECK(partial_ws->numel() >=
                (int64_t)B * Hq * nsplit * (D + 2),
                "partial_ws too small");
    ws = (float*)partial_ws->data_ptr();
  }
  if (kvq)
    TORCH_CHECK(k_scale->numel() >= (int64_t)B * Hkv * Smax &&
                v_scale->numel() >= (int64_t)B * Hkv * Smax,
                "scale tensors too small");
  launch_attn_decode(o.data_ptr(), q.data_ptr(), kc.data_ptr(),
                     vc.data_ptr(),
                     kvq ? k_scale->data_ptr() : nullptr,
                     kvq ? v_scale->data_ptr() : nullptr,
                     seq_lens.data_ptr(), B, Hq, Hkv, Smax,
                     (float)scale, q_row_stride, ws, (int)nsplit, stream());
}

void kv_append(torch::Tensor kc, torch::Tensor vc, torch::Tensor knew,
               torch::Tensor vnew, torch::Tensor positions) {
  CHECK_DEV(kc); CHECK_CONTIG(kc); CHECK_BF16(kc);
  CHECK_DEV(knew); CHECK_BF16(knew);
  CHECK_DEV(positions); CHECK_CONTIG(positions); CHECK_I32(positions);
  long long src_stride = check_head_view(knew);
  TORCH_CHECK(check_head_view(vnew) == src_stride,
              "knew/vnew strides must match");
  int B = kc.size(0), Hkv = kc.size(1), Smax = kc.size(2), D = kc.size(3);
  TORCH_CHECK(D % 8 == 0, "head_dim must be a multiple of 8");
  launch_kv_append(kc.data_ptr(), vc.data_ptr(), knew.data_ptr(),
                   vnew.data_ptr(), positions.data_ptr(), B, Hkv, Smax, D,
                   src_stride, stream());
}

// packed prefill: rope(q,k) in place + KV append at
// cache[tok_slot[t], :, positions[t]] for every packed token t
void rope_kv_varlen(torch::Tensor qkv, torch::Tensor kc, torch::Tensor vc,
                    torch::Tensor positions, torch::Tensor tok_slot,
                    torch::Tensor cos_sin, int64_t hq) {
  CHECK_DEV(qkv); CHECK_CONTIG(qkv); CHECK_BF16(qkv);
  CHECK_DEV(kc); CHECK_CONTIG(kc); CHECK_BF16(kc);
  CHECK_DEV(vc); CHECK_CONTIG(vc); CHECK_BF16(vc);
  CHECK_DEV(positions); CHECK_CONTIG(positions); CHECK_I32(positions);
  CHECK_DEV(tok_slot); CHECK_CONTIG(tok_slot); CHECK_I32(tok_slot);
  CHECK_DEV(cos_sin); CHECK_CONTIG(cos_sin); CHECK_F32(cos_sin);
  TORCH_CHECK(kc.dim() == 4 && vc.sizes() == kc.sizes(),
              "caches must be [B, Hkv, Smax, D] of equal shape");
  int B = kc.size(0), Hkv = kc.size(1), Smax = kc.size(2), D = kc.size(3);
  TORCH_CHECK(qkv.dim() == 2, "qkv must be [T, rows]");
  int64_t T = qkv.size(0);
  TORCH_CHECK(hq >= 1 && qkv.size(1) >= (hq + 2 * Hkv) * D,
              "qkv row too small");
  TORCH_CHECK(D % 2 == 0 && D / 2 <= 1024, "bad head dim");
  TORCH_CHECK(positions.numel() == T && tok_slot.numel() == T,
              "positions/tok_slot must hold one entry per token");
  TORCH_CHECK(cos_sin.dim() == 3 && cos_sin.size(1) == D / 2 &&
              cos_sin.size(2) == 2, "cos_sin must be [max_pos, D/2, 2]");
  TORCH_CHECK(hq + 2 * Hkv <= 65535, "too many heads");
  if (T == 0) return;
  launch_rope_kv_varlen(qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                        positions.data_ptr(), tok_slot.data_ptr(),
                        cos_sin.data_ptr(), (int)T, B, (int)hq, Hkv, Smax, D,
                        (int)cos_sin.size(0), qkv.size(1), stream());
}

// prefix cache: copy 32-token KV blocks src[:, src_row, :, src_blk*32..]
// -> dst[:, dst_row, :, dst_blk*32..] for every layer and KV head
void kv_block_copy(torch::Tensor src_k, torch::Tensor src_v,
                   torch::Tensor dst_k, torch::Tensor dst_v,
                   torch::Tensor src_row, torch::Tensor src_blk,
                   torch::Tensor dst_row, torch::Tensor dst_blk) {
  CHECK_DEV(src_k); CHECK_CONTIG(src_k); CHECK_BF16(src_k);
  CHECK_DEV(src_v); CHECK_CONTIG(src_v); CHECK_BF16(src_v);
  CHECK_DEV(dst_k); CHECK_CONTIG(dst_k); CHECK_BF16(dst_k);
  CHECK_DEV(dst_v); CHECK_CONTIG(dst_v); CHECK_BF16(dst_v);
  CHECK_DEV(src_row); CHECK_CONTIG(src_row); CHECK_I32(src_row);
  CHECK_DEV(src_blk); CHECK_CONTIG(src_blk); CHECK_I32(src_blk);
  CHECK_DEV(dst_row); CHECK_CONTIG(dst_row); CHECK_I32(dst_row);
  CHECK_DEV(dst_blk); CHECK_CONTIG(dst_blk); CHECK_I32(dst_blk);
  TORCH_CHECK(src_k.dim() == 5 && src_v.sizes() == src_k.sizes(),
              "src must be [L, Rs, Hkv, Ss, D] of equal shape");
  TORCH_CHECK(dst_k.dim() == 5 && dst_v.sizes() == dst_k.sizes(),
              "dst must be [L, Rd, Hkv, Sd, D] of equal shape");
  int64_t L = src_k.size(0), Hkv = src_k.size(2), D = src_k.size(4);
  TORCH_CHECK(dst_k.size(0) == L && dst_k.size(2) == Hkv &&
              dst_k.size(4) == D, "src/dst L, Hkv, D must match");
  TORCH_CHECK(D % 8 == 0, "head_dim * 2 bytes must be a multiple of 16");
  TORCH_CHECK(L * Hkv >= 1 && L * Hkv <= 65535, "too many layers*heads");
  int64_t n = src_row.numel();
  TORCH_CHECK(src_row.dim() == 1 && src_blk.dim() == 1 &&
              dst_row.dim() == 1 && dst_blk.dim() == 1 &&
              src_blk.numel() == n && dst_row.numel() == n &&
              dst_blk.numel() == n,
              "index vectors must be 1-d of equal length");
  TORCH_CHECK(src_k.size(1) <= INT_MAX && src_k.size(3) <= INT_MAX &&
              dst_k.size(1) <= INT_MAX && dst_k.size(3) <= INT_MAX &&
              n <= INT_MAX, "dimension too large");
  if (n == 0) return;
  launch_kv_block_copy(src_k.data_ptr(), src_v.data_ptr(), dst_k.data_ptr(),
                       dst_v.data_ptr(), src_row.data_ptr(),
                       src_blk.data_ptr(), dst_row.data_ptr(),
                       dst_blk.data_ptr(), (int)n, (int)L, (int)Hkv,
                       (int)src_k.size(1), (int)src_k.size(3),
                       (int)dst_k.size(1), (int)dst_k.size(3), (int)D,
                       stream());
}

// packed prefill: causal GQA flash attention over the slot-indexed cache
void attn_prefill(torch::Tensor o, torch::Tensor q, torch::Tensor kc,
                  torch::Tensor vc, torch::Tensor cu_seqlens,
                  torch::Tensor slots, torch::Tensor kv_start, double scale,
                  int64_t max_q_len) {
  CHECK_DEV(o); CHECK_CONTIG(o); CHECK_BF16(o);
  CHECK_DEV(q); CHECK_BF16(q);
  CHECK_DEV(kc); CHECK_CONTIG(kc); CHECK_BF16(kc);
  CHECK_DEV(vc); CHECK_CONTIG(vc); CHECK_BF16(vc);
  CHECK_DEV(cu_seqlens); CHECK_CONTIG(cu_seqlens); CHECK_I32(cu_seqlens);
  CHECK_DEV(slots); CHECK_CONTIG(slots); CHECK_I32(slots);
  CHECK_DEV(kv_start); CHECK_CONTIG(kv_start); CHECK_I32(kv_start);
  TORCH_CHECK(kc.dim() == 4 && vc.sizes() == kc.sizes(),
              "caches must be [B, Hkv, Smax, D] of equal shape");
  long long q_row_stride = check_head_view(q);
  int64_t T = q.size(0);
  int Hq = q.size(1), D = q.size(2);
  int B = kc.size(0), Hkv = kc.size(1), Smax = kc.size(2);
  TORCH_CHECK(D == 128 && kc.size(3) == D,
              "attn_prefill requires head_dim 128");
  TORCH_CHECK(Hq % Hkv == 0 && Hq / Hkv <= 8,
              "grouped heads per kv head must divide and be <= 8");
  TORCH_CHECK(o.numel() == T * Hq * D, "out must be [T, Hq*D]");
  // the kernel reads q and the caches with 16 B vector loads
  TORCH_CHECK(q_row_stride % 8 == 0 &&
              reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0,
              "q rows must be 16-byte aligned");
  int64_t nseq = slots.numel();
  TORCH_CHECK(cu_seqlens.numel() == nseq + 1 && kv_start.numel() == nseq,
              "cu_seqlens [n+1], slots [n], kv_start [n]");
  TORCH_CHECK(nseq <= 65535 && Hq <= 65535, "grid too large");
  TORCH_CHECK(max_q_len >= 0 && max_q_len <= T, "bad max_q_len");
  if (T == 0 || nseq == 0 || max_q_len == 0) return;
  launch_attn_prefill(o.data_ptr(), q.data_ptr(), kc.data_ptr(),
                      vc.data_ptr(), cu_seqlens.data_ptr(),
                      slots.data_ptr(), kv_start.data_ptr(), (int)T,
                      (int)nseq, B, Hq, Hkv, Smax, (float)scale,
                      q_row_stride, (int)max_q_len, stream());
}

// speculative verify: QL query rows per sequence against the cached
// prefix; q [B, QL, Hq, D] may be a strided view into the qkv buffer
void attn_verify(torch::Tensor o, torch::Tensor q, torch::Tensor kc,
                 torch::Tensor vc, torch::Tensor base_lens, double scale,
                 c10::optional<torch::Tensor> partial_ws, int64_t nsplit) {
  CHECK_DEV(o); CHECK_CONTIG(o); CHECK_BF16(o);
  CHECK_DEV(q); CHECK_BF16(q);
  CHECK_DEV(kc); CHECK_CONTIG(kc); CHECK_BF16(kc);
  CHECK_DEV(vc); CHECK_CONTIG(vc); CHECK_BF16(vc);
  CHECK_DEV(base_lens); CHECK_CONTIG(base_lens); CHECK_I32(base_lens);
  TORCH_CHECK(q.dim() == 4, "q must be [B, QL, Hq, D]");
  TORCH_CHECK(kc.dim() == 4 && vc.sizes() == kc.sizes(),
              "caches must be [B, Hkv, Smax, D] of equal shape");
  int64_t B = q.size(0);
  int QL = q.size(1), Hq = q.size(2), D = q.size(3);
  int Hkv = kc.size(1), Smax = kc.size(2);
  TORCH_CHECK(D == 128 && kc.size(3) == D,
              "attn_verify requires head_dim 128");
  TORCH_CHECK(QL >= 1 && QL <= 8, "attn_verify needs 1 <= QL <= 8");
  TORCH_CHECK(Hkv >= 1 && Hq % Hkv == 0 && Hq / Hkv <= 8,
              "grouped heads per kv head must divide and be <= 8");
  TORCH_CHECK(kc.size(0) == B && base_lens.numel() == B,
              "q, caches and base_lens must agree on B");
  TORCH_CHECK(q.stride(3) == 1 && q.stride(2) == D,
              "inner dims must be dense (strides (*, *, dim, 1))");
  // a size-1 dim has no meaningful stride: take the row stride from
  // the dim that really steps through the rows
  long long q_row_stride = QL > 1 ? q.stride(1) : q.stride(0);
  if (B == 1 && QL == 1) q_row_stride = (long long)Hq * D;
  TORCH_CHECK(QL == 1 || B == 1 || q.stride(0) == QL * q.stride(1),
              "q rows must be evenly strided over [B, QL]");
  TORCH_CHECK(q_row_stride >= (long long)Hq * D,
              "q rows must not overlap");
  // the kernel reads q and the caches with 16 B vector loads
  TORCH_CHECK(q_row_stride % 8 == 0 &&
              reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0,
              "q rows must be 16-byte aligned");
  TORCH_CHECK(o.numel() == B * QL * Hq * D, "out must be [B*QL, Hq*D]");
  TORCH_CHECK(B <= 65535 && Hkv <= 65535, "grid too large");
  TORCH_CHECK(nsplit >= 1 && nsplit <= 1024, "bad nsplit");
  float* ws = nullptr;
  if (nsplit > 1) {
    TORCH_CHECK(partial_ws.has_value(), "nsplit>1 needs partial_ws");
    CHECK_DEV(*partial_ws); CHECK_CONTIG(*partial_ws);
    CHECK_F32(*partial_ws);
    TORCH_CHECK(partial_ws->numel() >=
                B * QL * Hq * nsplit * (int64_t)(D + 4),
                "partial_ws too small");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(partial_ws->data_ptr()) % 16
                == 0, "partial_ws must be 16-byte aligned");
    ws = (float*)partial_ws->data_ptr();
  }
  if (B == 0) return;
  launch_attn_verify(o.data_ptr(), q.data_ptr(), kc.data_ptr(),
                     vc.data_ptr(), base_lens.data_ptr(), (int)B, QL, Hq,
                     Hkv, Smax, (float)scale, q_row_stride, ws,
                     (int)nsplit, stream());
}

// device-side prompt-lookup drafter
void ngram_draft(torch::Tensor drafts, torch::Tensor history,
                 torch::Tensor hist_lens, int64_t n) {
  CHECK_DEV(drafts); CHECK_CONTIG(drafts);
  CHECK_DEV(history); CHECK_CONTIG(history);
  CHECK_DEV(hist_lens); CHECK_CONTIG(hist_lens); CHECK_I32(hist_lens);
  TORCH_CHECK(drafts.scalar_type() == torch::kInt64 &&
              history.scalar_type() == torch::kInt64,
              "drafts and history must be int64");
  TORCH_CHECK(history.dim() == 2 && drafts.dim() == 2,
              "history [B, L], drafts [B, k]");
  int64_t B = history.size(0), L = history.size(1), k = drafts.size(1);
  TORCH_CHECK(drafts.size(0) == B && hist_lens.numel() == B,
              "drafts, history and hist_lens must agree on B");
  TORCH_CHECK(n >= 1 && n <= 64, "ngram_draft needs 1 <= n <= 64");
  TORCH_CHECK(L < (1LL << 30) && k < (1LL << 20), "shape too large");
  if (B == 0 || k == 0) return;
  launch_ngram_draft(drafts.data_ptr(), history.data_ptr(),
                     hist_lens.data_ptr(), (int)B, (int)L, (int)k, (int)n,
                     stream());
}

// multi-LoRA decode (BGMV): shared shape checks of the two kernels
static void check_lora(const torch::Tensor& act, const torch::Tensor& t,
                       const torch::Tensor& table, const torch::Tensor& idx,
                       int64_t width, const char* width_name) {
  TORCH_CHECK(act.dim() == 2 && t.dim() == 2 && table.dim() == 3 &&
              idx.dim() == 1, "lora: expected 2-d rows, t [B, R], a "
              "[NA, ., .] table and idx [B]");
  int64_t B = act.size(0), R = t.size(1);
  TORCH_CHECK(B <= 64, "lora: at most 64 rows, got ", B);
  TORCH_CHECK(t.size(0) == B && idx.numel() == B,
              "lora: rows, t and idx must agree on B");
  TORCH_CHECK(R == 8 || R == 16 || R == 32 || R == 64,
              "lora: rank must be 8, 16, 32 or 64, got ", R);
  TORCH_CHECK(width % 8 == 0, "lora: ", width_name,
              " must be a multiple of 8, got ", width);
  TORCH_CHECK(table.size(0) < (1LL << 20) && width < (1LL << 24),
              "lora: shape too large");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(act.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(table.data_ptr()) % 16 == 0,
              "lora: rows and tables must be 16-byte aligned");
}

void lora_shrink(torch::Tensor t, torch::Tensor x, torch::Tensor A,
                 torch::Tensor idx) {
  CHECK_DEV(t); CHECK_CONTIG(t); CHECK_F32(t);
  CHECK_DEV(x); CHECK_CONTIG(x); CHECK_BF16(x);
  CHECK_DEV(A); CHECK_CONTIG(A); CHECK_BF16(A);
  CHECK_DEV(idx); CHECK_CONTIG(idx); CHECK_I32(idx);
  check_lora(x, t, A, idx, x.dim() == 2 ? x.size(1) : 0, "K");
  TORCH_CHECK(A.size(1) == t.size(1) && A.size(2) == x.size(1),
              "lora_shrink: A must be [NA, R, K]");
  launch_lora_shrink(t.data_ptr(), x.data_ptr(), A.data_ptr(),
                     idx.data_ptr(), (int)x.size(0), (int)A.size(0),
                     (int)t.size(1), (int)x.size(1), stream());
}

void lora_expand(torch::Tensor y, torch::Tensor t, torch::Tensor Bm,
                 torch::Tensor idx) {
  CHECK_DEV(y); CHECK_CONTIG(y); CHECK_BF16(y);
  CHECK_DEV(t); CHECK_CONTIG(t); CHECK_F32(t);
  CHECK_DEV(Bm); CHECK_CONTIG(Bm); CHECK_BF16(Bm);
  CHECK_DEV(idx); CHECK_CONTIG(idx); CHECK_I32(idx);
  check_lora(y, t, Bm, idx, y.dim() == 2 ? y.size(1) : 0, "N");
  TORCH_CHECK(Bm.size(1) == y.size(1) && Bm.size(2) == t.size(1),
              "lora_expand: Bm must be [NA, N, R]");
  launch_lora_expand(y.data_ptr(), t.data_ptr(), Bm.data_ptr(),
                     idx.data_ptr(), (int)y.size(0), (int)Bm.size(0),
                     (int)t.size(1), (int)y.size(1), stream());
}

// fused per-request sampler: one workgroup per logits row
void sample_tokens(torch::Tensor logits, torch::Tensor pos,
                   torch::Tensor temperature, torch::Tensor top_k,
                   torch::Tensor top_p, torch::Tensor min_p,
                   torch::Tensor seed, torch::Tensor out_tokens,
                   c10::optional<torch::Tensor> out_logprob,
                   c10::optional<torch::Tensor> out_kept) {
  CHECK_DEV(logits); CHECK_CONTIG(logits); CHECK_BF16(logits);
  CHECK_DEV(pos); CHECK_CONTIG(pos); CHECK_I32(pos);
  CHECK_DEV(temperature); CHECK_CONTIG(temperature); CHECK_F32(temperature);
  CHECK_DEV(top_k); CHECK_CONTIG(top_k); CHECK_I32(top_k);
  CHECK_DEV(top_p); CHECK_CONTIG(top_p); CHECK_F32(top_p);
  CHECK_DEV(min_p); CHECK_CONTIG(min_p); CHECK_F32(min_p);
  CHECK_DEV(seed); CHECK_CONTIG(seed);
  CHECK_DEV(out_tokens); CHECK_CONTIG(out_tokens);
  TORCH_CHECK(seed.scalar_type() == torch::kInt64 &&
              out_tokens.scalar_type() == torch::kInt64,
              "sample_tokens: seed and out_tokens must be int64");
  TORCH_CHECK(logits.dim() == 2, "sample_tokens: logits must be [B, V]");
  const int64_t B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(B <= 64, "sample_tokens: at most 64 rows, got ", B);
  TORCH_CHECK(V % 8 == 0 && V < (1LL << 24),
              "sample_tokens: V must be a multiple of 8 below 2^24, got ", V);
  TORCH_CHECK(pos.numel() == B && temperature.numel() == B &&
              top_k.numel() == B && top_p.numel() == B &&
              min_p.numel() == B && seed.numel() == B &&
              out_tokens.numel() == B,
              "sample_tokens: every per-row tensor must hold B entries");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(logits.data_ptr()) % 16 == 0,
              "sample_tokens: logits must be 16-byte aligned");
  void* logprob_ptr = nullptr;
  void* kept_ptr = nullptr;
  if (out_logprob.has_value()) {
    CHECK_DEV(*out_logprob); CHECK_CONTIG(*out_logprob);
    CHECK_F32(*out_logprob);
    TORCH_CHECK(out_logprob->numel() == B,
                "sample_tokens: out_logprob must hold B entries");
    logprob_ptr = out_logprob->data_ptr();
  }
  if (out_kept.has_value()) {
    CHECK_DEV(*out_kept); CHECK_CONTIG(*out_kept); CHECK_I32(*out_kept);
    TORCH_CHECK(out_kept->numel() == B,
                "sample_tokens: out_kept must hold B entries");
    kept_ptr = out_kept->data_ptr();
  }
  if (B == 0) return;
  launch_sample_tokens(logits.data_ptr(), pos.data_ptr(),
                       temperature.data_ptr(), top_k.data_ptr(),
                       top_p.data_ptr(), min_p.data_ptr(), seed.data_ptr(),
                       out_tokens.data_ptr(), logprob_ptr, kept_ptr, (int)B,
                       (int)V, stream());
}

// penalties and logit bias in place on the logits, from the per-slot
// token-state table that the same kernel maintains
void logit_processors(torch::Tensor logits, torch::Tensor state,
                      torch::Tensor penalties, torch::Tensor bias_ids,
                      torch::Tensor bias_val, torch::Tensor bias_n,
                      c10::optional<torch::Tensor> tokens,
                      c10::optional<torch::Tensor> rows) {
  CHECK_DEV(logits); CHECK_CONTIG(logits); CHECK_BF16(logits);
  CHECK_DEV(state); CHECK_CONTIG(state); CHECK_I32(state);
  CHECK_DEV(penalties); CHECK_CONTIG(penalties); CHECK_F32(penalties);
  CHECK_DEV(bias_ids); CHECK_CONTIG(bias_ids); CHECK_I32(bias_ids);
  CHECK_DEV(bias_val); CHECK_CONTIG(bias_val); CHECK_F32(bias_val);
  CHECK_DEV(bias_n); CHECK_CONTIG(bias_n); CHECK_I32(bias_n);
  TORCH_CHECK(logits.dim() == 2 && state.dim() == 2,
              "logit_processors: logits must be [B, V], state [S, V]");
  const int64_t B = logits.size(0), V = logits.size(1), S = state.size(0);
  TORCH_CHECK(B <= 64, "logit_processors: at most 64 rows, got ", B);
  TORCH_CHECK(V % 8 == 0 && V < (1LL << 24),
              "logit_processors: V must be a multiple of 8 below 2^24, got ",
              V);
  TORCH_CHECK(state.size(1) == V,
              "logit_processors: state must be [S, V] with the logits' V");
  TORCH_CHECK(penalties.dim() == 2 && penalties.size(0) == B &&
              penalties.size(1) == 3,
              "logit_processors: penalties must be [B, 3]");
  TORCH_CHECK(bias_ids.dim() == 2 && bias_ids.size(0) == B &&
              bias_ids.size(1) == 64 && bias_val.dim() == 2 &&
              bias_val.size(0) == B && bias_val.size(1) == 64,
              "logit_processors: bias_ids and bias_val must be [B, 64]");
  TORCH_CHECK(bias_n.numel() == B,
              "logit_processors: bias_n must hold B entries");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(logits.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(state.data_ptr()) % 16 == 0,
              "logit_processors: logits and state must be 16-byte aligned");
  const void* tokens_ptr = nullptr;
  const void* rows_ptr = nullptr;
  if (tokens.has_value()) {
    CHECK_DEV(*tokens); CHECK_CONTIG(*tokens);
    TORCH_CHECK(tokens->scalar_type() == torch::kInt64 &&
                tokens->numel() == B,
                "logit_processors: tokens must be int64 [B]");
    tokens_ptr = tokens->data_ptr();
  }
  if (rows.has_value()) {
    CHECK_DEV(*rows); CHECK_CONTIG(*rows); CHECK_I32(*rows);
    TORCH_CHECK(rows->numel() == B,
                "logit_processors: rows must hold B entries");
    rows_ptr = rows->data_ptr();
  }
  if (B == 0 || S == 0) return;
  launch_logit_processors(logits.data_ptr(), state.data_ptr(),
                          penalties.data_ptr(), bias_ids.data_ptr(),
                          bias_val.data_ptr(), bias_n.data_ptr(), tokens_ptr,
                          rows_ptr, (int)B, (int)V, (int)S, stream());
}

void softmax(torch::Tensor out, torch::Tensor in) {
  CHECK_DEV(out); CHECK_CONTIG(out); CHECK_BF16(out);
  CHECK_DEV(in); CHECK_CONTIG(in); CHECK_BF16(in);
  int64_t cols = in.size(-1);
  int64_t rows = in.numel() / cols;
  launch_softmax(out.data_ptr(), in.data_ptr(), (int)rows, (int)cols,
                 stream());
}

void tree_ensemble(torch::Tensor out, torch::Tensor features,
                   torch::Tensor feature_idx, torch::Tensor threshold,
                   torch::Tensor left, torch::Tensor right,
                   torch::Tensor leaf_value, torch::Tensor tree_offsets,
                   double base_score) {
  CHECK_DEV(out); CHECK_CONTIG(out); CHECK_F32(out);
  CHECK_DEV(features); CHECK_CONTIG(features); CHECK_F32(features);
  CHECK_I32(feature_idx); CHECK_I32(left); CHECK_I32(right);
  CHECK_I32(tree_offsets); CHECK_F32(threshold); CHECK_F32(leaf_value);
  int n_samples = features.size(0), n_features = features.size(1);
  int n_trees = tree_offsets.numel() - 1;
  launch_tree_ensemble(out.data_ptr(), features.data_ptr(),
                       feature_idx.data_ptr(), threshold.data_ptr(),
                       left.data_ptr(), right.data_ptr(),
                       leaf_value.data_ptr(), tree_offsets.data_ptr(),
                       n_trees, n_samples, n_features, (float)base_score,
                       stream());
}

void window_ingest(torch::Tensor ring, torch::Tensor keys,
                   torch::Tensor values, torch::Tensor period_idx) {
  CHECK_DEV(ring); CHECK_CONTIG(ring);
  CHECK_I32(keys); CHECK_F32(values); CHECK_I32(period_idx);
  TORCH_CHECK(ring.dim() == 3 && ring.size(2) == 4,
              "ring must be [keys, periods, 4]");
  if (ring.scalar_type() == torch::kFloat64) {
    // f64 ring: sum-of-SQUARES accumulation (stdvar precision)
    launch_window_ingest64(ring.data_ptr(), keys.data_ptr(),
                           values.data_ptr(), period_idx.data_ptr(),
                           keys.numel(), (int)ring.size(1), stream());
    return;
  }
  CHECK_F32(ring);
  launch_window_ingest(ring.data_ptr(), keys.data_ptr(), values.data_ptr(),
                       period_idx.data_ptr(), keys.numel(),
                       (int)ring.size(1), stream());
}

void window_reduce(torch::Tensor out, torch::Tensor ring,
                   int64_t window_periods, int64_t current_period) {
  CHECK_DEV(out); CHECK_CONTIG(out);
  CHECK_DEV(ring); CHECK_CONTIG(ring);
  if (ring.scalar_type() == torch::kFloat64) {
    TORCH_CHECK(out.scalar_type() == torch::kFloat64,
                "out must be f64 for an f64 ring");
    launch_window_reduce64(out.data_ptr(), ring.data_ptr(),
                           (int)ring.size(0), (int)ring.size(1),
                           (int)window_periods, (int)current_period,
                           stream());
    return;
  }
  CHECK_F32(out); CHECK_F32(ring);
  launch_window_reduce(out.data_ptr(), ring.data_ptr(), (int)ring.size(0),
                       (int)ring.size(1), (int)window_periods,
                       (int)current_period, stream());
}

void window_ingest_mm(torch::Tensor ring_mm, torch::Tensor keys,
                      torch::Tensor values, torch::Tensor period_idx) {
  CHECK_DEV(ring_mm); CHECK_CONTIG(ring_mm);
  TORCH_CHECK(ring_mm.scalar_type() == torch::kInt32,
              "ring_mm must be int32 (ordered-f32 bits)");
  CHECK_I32(keys); CHECK_F32(values); CHECK_I32(period_idx);
  TORCH_CHECK(ring_mm.dim() == 3 && ring_mm.size(2) == 2,
              "ring_mm must be [keys, periods, 2]");
  launch_window_ingest_mm(ring_mm.data_ptr(), keys.data_ptr(),
                          values.data_ptr(), period_idx.data_ptr(),
                          keys.numel(), (int)ring_mm.size(1), stream());
}

void window_ingest_fl(torch::Tensor ring_fl, torch::Tensor keys,
                      torch::Tensor values, torch::Tensor timestamps,
                      torch::Tensor period_idx) {
  CHECK_DEV(ring_fl); CHECK_CONTIG(ring_fl);
  TORCH_CHECK(ring_fl.scalar_type() == torch::kInt64,
              "ring_fl must be int64 (packed ts|ordered-f32)");
  CHECK_I32(keys); CHECK_F32(values); CHECK_I32(timestamps);
  CHECK_I32(period_idx);
  TORCH_CHECK(ring_fl.dim() == 3 && ring_fl.size(2) == 2,
              "ring_fl must be [keys, periods, 2]");
  launch_window_ingest_fl(ring_fl.data_ptr(), keys.data_ptr(),
                          values.data_ptr(), timestamps.data_ptr(),
                          period_idx.data_ptr(), keys.numel(),
                          (int)ring_fl.size(1), stream());
}

void window_reduce_mmfl(torch::Tensor out, torch::Tensor ring_mm,
                        torch::Tensor ring_fl, int64_t window_periods,
                        int64_t current_period) {
  CHECK_DEV(out); CHECK_CONTIG(out); CHECK_F32(out);
  CHECK_DEV(ring_mm); CHECK_CONTIG(ring_mm);
  CHECK_DEV(ring_fl); CHECK_CONTIG(ring_fl);
  TORCH_CHECK(out.dim() == 2 && out.size(1) == 4,
              "out must be [keys, 4]");
  launch_window_reduce_mmfl(out.data_ptr(), ring_mm.data_ptr(),
                            ring_fl.data_ptr(), (int)ring_mm.size(0),
                            (int)ring_mm.size(1), (int)window_periods,
                            (int)current_period, stream());
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("fused_add_rmsnorm", &fused_add_rmsnorm,
        "fused residual add + RMSNorm (bf16)");
  m.def("rope", &rope, "in-place rotary embedding (bf16)");
  m.def("silu_mul", &silu_mul, "silu(gate) * up (bf16)");
  m.def("swiglu_fused", &swiglu_fused,
        "silu(gu[:, :I]) * gu[:, I:] over a fused gate|up buffer");
  m.def("skinny_gemm", &skinny_gemm,
        "decode GEMM C=A@W^T on MFMA (bf16 in/out, split-K f32 slabs)");
  m.def("rope_kv_fused", &rope_kv_fused, py::arg("qkv"), py::arg("kc"),
        py::arg("vc"), py::arg("positions"), py::arg("cos_sin"),
        py::arg("hq"), py::arg("k_scale") = py::none(),
        py::arg("v_scale") = py::none(),
        "fused decode rope(q,k) + KV-cache append");
  m.def("skinny_gemm_slabs", &skinny_gemm_slabs,
        "split-K GEMM emitting f32 slabs only");
  m.def("fused_add_rmsnorm_slab", &fused_add_rmsnorm_slab,
        "slab-sum + residual add + RMSNorm");
  m.def("swiglu_slab", &swiglu_slab, "slab-sum + SwiGLU");
  m.def("rope_kv_slab", &rope_kv_slab,
        "slab-sum + rope(q,k) + KV append");
  m.def("cast_f32_bf16", &cast_f32_bf16, "f32 -> bf16 cast");
  m.def("skinny_gemm_fp8", &skinny_gemm_fp8,
        "fp8-weight decode GEMM (e4m3, per-row scales)");
  m.def("quant_fp8_rows", &quant_fp8_rows,
        "dynamic per-row bf16 -> fp8 e4m3 quantization");
  m.def("attn_decode", &attn_decode, py::arg("o"), py::arg("q"),
        py::arg("kc"), py::arg("vc"), py::arg("seq_lens"),
        py::arg("scale"), py::arg("partial_ws") = py::none(),
        py::arg("nsplit") = 1, py::arg("k_scale") = py::none(),
        py::arg("v_scale") = py::none(),
        "GQA decode attention (bf16 or fp8 KV cache)");
  m.def("kv_append", &kv_append, "append token K/V into cache");
  m.def("rope_kv_varlen", &rope_kv_varlen, py::arg("qkv"), py::arg("kc"),
        py::arg("vc"), py::arg("positions"), py::arg("tok_slot"),
        py::arg("cos_sin"), py::arg("hq"),
        "packed-prefill rope(q,k) + KV append by per-token slot");
  m.def("kv_block_copy", &kv_block_copy, py::arg("src_k"),
        py::arg("src_v"), py::arg("dst_k"), py::arg("dst_v"),
        py::arg("src_row"), py::arg("src_blk"), py::arg("dst_row"),
        py::arg("dst_blk"),
        "prefix cache: copy 32-token KV blocks between pool and cache");
  m.def("attn_prefill", &attn_prefill, py::arg("o"), py::arg("q"),
        py::arg("kc"), py::arg("vc"), py::arg("cu_seqlens"),
        py::arg("slots"), py::arg("kv_start"), py::arg("scale"),
        py::arg("max_q_len"),
        "packed causal GQA flash-attention prefill over the KV cache");
  m.def("attn_verify", &attn_verify, py::arg("o"), py::arg("q"),
        py::arg("kc"), py::arg("vc"), py::arg("base_lens"),
        py::arg("scale"), py::arg("partial_ws") = py::none(),
        py::arg("nsplit") = 1,
        "speculative verify attention (QL query rows per sequence)");
  m.def("ngram_draft", &ngram_draft, py::arg("drafts"), py::arg("history"),
        py::arg("hist_lens"), py::arg("n"),
        "device-side prompt-lookup (n-gram) drafter");
  m.def("lora_shrink", &lora_shrink, py::arg("t"), py::arg("x"),
        py::arg("a"), py::arg("idx"),
        "multi-LoRA shrink: t[b] = A[idx[b]] @ x[b] (f32)");
  m.def("lora_expand", &lora_expand, py::arg("y"), py::arg("t"),
        py::arg("bm"), py::arg("idx"),
        "multi-LoRA expand: y[b] += Bm[idx[b]] @ t[b], in place (bf16)");
  m.def("sample_tokens", &sample_tokens, py::arg("logits"), py::arg("pos"),
        py::arg("temperature"), py::arg("top_k"), py::arg("top_p"),
        py::arg("min_p"), py::arg("seed"), py::arg("out_tokens"),
        py::arg("out_logprob") = py::none(),
        py::arg("out_kept") = py::none(),
        "fused seeded sampler: temperature, top_k, top_p, min_p, logprob");
  m.def("logit_processors", &logit_processors, py::arg("logits"),
        py::arg("state"), py::arg("penalties"), py::arg("bias_ids"),
        py::arg("bias_val"), py::arg("bias_n"),
        py::arg("tokens") = py::none(), py::arg("rows") = py::none(),
        "repetition / presence / frequency penalties and logit bias, in "
        "place, with the per-slot token counts");
  m.def("softmax", &softmax, "row softmax (bf16)");
  m.def("tree_ensemble", &tree_ensemble, "GBDT ensemble inference (f32)");
  m.def("window_ingest", &window_ingest,
        "feature-store window ring ingest (f32)");
  m.def("window_reduce", &window_reduce,
        "feature-store window ring reduce (f32)");
  m.def("window_ingest_mm", &window_ingest_mm,
        "per-period min/max ingest (ordered-f32 atomics)");
  m.def("window_ingest_fl", &window_ingest_fl,
        "per-period first/last ingest (packed ts|value u64 atomics)");
  m.def("window_reduce_mmfl", &window_reduce_mmfl,
        "window min/max/first/last reduce over period cells");
}
