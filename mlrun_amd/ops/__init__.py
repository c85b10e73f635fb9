# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""GPU ops: python dispatch over the in-tree HIP extension
(mlrun_amd._hip_ops, built from ops/hip/kernels.hip for gfx950).

Dispatch policy:
- tensors on GPU  -> the HIP extension MUST be present; a missing
  extension raises MLRunGPUError loudly (no silent eager fallback)
- tensors on CPU  -> plain fp32 torch reference implementations (these
  are also the ground truth the GPU numerics tests compare against)
"""

import math
import os

import torch

from ..errors import MLRunGPUError

try:
    from mlrun_amd import _hip_ops  # built in-tree by setup.py

    HAVE_HIP_OPS = True
except ImportError:
    _hip_ops = None
    HAVE_HIP_OPS = False


def _require_hip():
    if not HAVE_HIP_OPS:
        raise MLRunGPUError(
            "mlrun_amd._hip_ops extension is not built — run "
            "`PYTORCH_ROCM_ARCH=gfx950 python setup.py build_ext --inplace` "
            "(GPU ops never fall back to eager execution)")
    return _hip_ops


# ------------------------------------------------------------------ norm


def fused_add_rmsnorm(x: torch.Tensor, weight: torch.Tensor,
                      residual: torch.Tensor = None, eps: float = 1e-5,
                      out: torch.Tensor = None,
                      out8: torch.Tensor = None,
                      out_scale: torch.Tensor = None) -> torch.Tensor:
    """out = rmsnorm(x + residual) * weight; residual <- x + residual
    (in-place) when given.  out8/out_scale: also emit the fp8
    pair-swizzled quantization of the output (fp8-weight decode)."""
    if x.is_cuda:
        ops = _require_hip()
        if out is None:
            out = torch.empty_like(x)
        ops.fused_add_rmsnorm(out, x, weight, residual, eps, out8,
                              out_scale)
        return out
    # fp32 reference
    z = x.float() + (residual.float() if residual is not None else 0.0)
    var = z.pow(2).mean(dim=-1, keepdim=True)
    if residual is not None:
        # as the kernel does: the sum of squares takes the fp32 sum,
        # the normalization the new residual as stored
        residual.copy_(z.to(residual.dtype))
        z = residual.float()
    result = (z * torch.rsqrt(var + eps)) * weight.float()
    result = result.to(x.dtype)
    if out is not None:
        out.copy_(result)
        return out
    return result


def rmsnorm(x, weight, eps=1e-5, out=None, out8=None, out_scale=None):
    return fused_add_rmsnorm(x, weight, residual=None, eps=eps, out=out,
                             out8=out8, out_scale=out_scale)


# ------------------------------------------------------------------ rope


def build_rope_cos_sin(max_pos: int, head_dim: int, theta: float = 500000.0,
                       device="cpu") -> torch.Tensor:
    """Precompute the [max_pos, head_dim/2, 2] f32 cos/sin table
    (host-side trig — guide Appendix B)."""
    half = head_dim // 2
    inv_freq = 1.0 / (theta ** (torch.arange(0, half, dtype=torch.float64)
                                / half))
    pos = torch.arange(max_pos, dtype=torch.float64)
    angles = torch.outer(pos, inv_freq)  # [max_pos, half]
    table = torch.stack([angles.cos(), angles.sin()], dim=-1).float()
    return table.contiguous().to(device)


def rope_inplace(q: torch.Tensor, positions: torch.Tensor,
                 cos_sin: torch.Tensor):
    """In-place neox-style rotary embedding. q: [T, heads, dim]."""
    if q.is_cuda:
        _require_hip().rope(q, positions, cos_sin)
        return q
    T, heads, dim = q.shape
    half = dim // 2
    table = cos_sin[positions.long()]  # [T, half, 2]
    cos = table[..., 0].unsqueeze(1)  # [T,1,half]
    sin = table[..., 1].unsqueeze(1)
    qf = q.float()
    q1 = qf[..., :half]
    q2 = qf[..., half:]
    q[..., :half] = (q1 * cos - q2 * sin).to(q.dtype)
    q[..., half:] = (q2 * cos + q1 * sin).to(q.dtype)
    return q


# ---------------------------------------------------------------- swiglu


def swiglu_fused(gu: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """silu(gu[:, :I]) * gu[:, I:] over the fused gate|up projection."""
    rows, two_i = gu.shape
    inter = two_i // 2
    if gu.is_cuda:
        ops = _require_hip()
        if out is None:
            out = torch.empty(rows, inter, dtype=gu.dtype, device=gu.device)
        ops.swiglu_fused(out, gu)
        return out
    result = (torch.nn.functional.silu(gu[:, :inter].float()) *
              gu[:, inter:].float()).to(gu.dtype)
    if out is not None:
        out.copy_(result)
        return out
    return result


def silu_mul(gate: torch.Tensor, up: torch.Tensor,
             out: torch.Tensor = None) -> torch.Tensor:
    if gate.is_cuda:
        ops = _require_hip()
        if out is None:
            out = torch.empty_like(gate)
        ops.silu_mul(out, gate, up)
        return out
    result = (torch.nn.functional.silu(gate.float()) *
              up.float()).to(gate.dtype)
    if out is not None:
        out.copy_(result)
        return out
    return result


# ------------------------------------------------------------------ gemm


def pick_ksplit(M: int, N: int, K: int, target_blocks: int = 2048) -> int:
    """Choose the K-split so the grid fills 256 CUs (~2048 wgs)."""
    nblocks = (N + 127) // 128
    if nblocks >= target_blocks:
        return 1
    ksplit = (target_blocks + nblocks - 1) // nblocks
    ksplit = min(ksplit, max(K // 256, 1), 16)
    return max(ksplit, 1)


_EMPTY_F32 = None


# measured on MI355X (scripts/bench_gemm.py sweep, profiles/): best
# (ksplit, variant) per llama projection shape; variant 1/2 = wave-split
_GEMM_PLAN_TABLE = {
    # NOTE: plans are tuned against the END-TO-END bench, not the
    # standalone sweep — even the L3-honest sweep (rotated weights)
    # picks cells that regress the bench by ~6% (in-graph execution
    # state differs: back-to-back kernels, dirty L2, sustained clocks).
    # Three e2e A/Bs confirmed this table; treat e2e as ground truth.
    # Variant 4 = LDS-DMA operand rings (batch 17..32; other batch
    # sizes run variant 1's kernels).  All four projections moved from
    # variant 2 at UNCHANGED ksplit, so outputs are bit-identical:
    # e2e 149.2 -> 191.8 req/s (medians of 3 alternating runs); every
    # shape gains alone except qkv (neutral alone, +1.3% on top of the
    # other three).  ksplit re-tunes at variant 4 (qkv 2, wo 1/4,
    # gate|up 2, down 2/8) were all within +-1.5% or worse: not taken.
    (6144, 4096): (4, 4),     # qkv (ks4: 768 WGs vs 192 — re-tuned
    #   after the attention/LDS round; e2e 126.4 -> 127.9 req/s)
    (4096, 4096): (2, 4),     # wo
    (28672, 4096): (1, 4),    # gate|up
    (4096, 14336): (4, 4),    # down
    (128256, 4096): (1, 0),   # lm_head
}

# e2e A/B override: MLRUN_GEMM_PLAN="6144x4096=2,2;4096x4096=4,2"
_plan_env = os.environ.get("MLRUN_GEMM_PLAN", "")
if _plan_env:
    for _cell in _plan_env.split(";"):
        _shape, _plan = _cell.split("=")
        _n, _k = _shape.split("x")
        _ks, _var = _plan.split(",")
        _GEMM_PLAN_TABLE[(int(_n), int(_k))] = (int(_ks), int(_var))


def pick_gemm_plan(M: int, N: int, K: int) -> tuple:
    """(ksplit, variant): variant 1 = wave-split-K (4 waves share one
    32-wide n-tile) for small-N projections, else the 128-wide tiler.
    Known llama shapes use the measured sweep table."""
    if (N, K) in _GEMM_PLAN_TABLE:
        return _GEMM_PLAN_TABLE[(N, K)]
    nblocks_ws = (N + 31) // 32
    if nblocks_ws <= 512 and K >= 2048:
        # small-N: wave-split for 4x waves/SIMD at equal slab traffic
        ksplit = max(1, min(1024 // nblocks_ws, K // 1024, 8))
        return ksplit, 1
    return pick_ksplit(M, N, K), 0


def skinny_gemm(a: torch.Tensor, w: torch.Tensor,
                out: torch.Tensor = None,
                c_f32: torch.Tensor = None,
                ksplit: int = None, variant: int = None) -> torch.Tensor:
    """C[M,N] = A[M,K] @ W[N,K]^T for decode batches (M <= 32), bf16.

    On GPU: MFMA kernel; split-K writes per-chunk f32 slabs into c_f32
    and a reduce kernel folds them to bf16 (deterministic, no atomics).
    Pass preallocated out/c_f32 for graph capture."""
    global _EMPTY_F32

    M, K = a.shape
    N = w.shape[0]
    if a.is_cuda:
        ops = _require_hip()
        if ksplit is None and variant is None:
            ksplit, variant = pick_gemm_plan(M, N, K)
        elif ksplit is None:
            ksplit = pick_ksplit(M, N, K)
        elif variant is None:
            variant = 0
        if out is None:
            out = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
        if ksplit > 1 and c_f32 is None:
            c_f32 = torch.empty(ksplit * M * N, dtype=torch.float32,
                                device=a.device)
        if c_f32 is None:
            if _EMPTY_F32 is None or _EMPTY_F32.device != a.device:
                _EMPTY_F32 = torch.empty(1, dtype=torch.float32,
                                         device=a.device)
            c_f32 = _EMPTY_F32
        ops.skinny_gemm(out, c_f32, a, w, ksplit, variant)
        return out
    result = (a.float() @ w.float().t()).to(a.dtype)
    if out is not None:
        out.copy_(result)
        return out
    return result


FP8_MAX = 448.0  # OCP e4m3 max normal


def _fp8_pair_swizzle(q: torch.Tensor) -> torch.Tensor:
    """[N, K] -> pair-swizzled layout so a lane's 16B load carries two
    K-steps (kernel layout: new[(s/2)*64 + c*16 + (s%2)*8 + j])."""
    n, k = q.shape
    assert k % 64 == 0, "K must be a multiple of 64 for the fp8 path"
    return q.view(n, k // 64, 2, 4, 8).permute(0, 1, 3, 2, 4) \
        .contiguous().view(n, k)


def _fp8_pair_unswizzle(q: torch.Tensor) -> torch.Tensor:
    n, k = q.shape
    return q.view(n, k // 64, 4, 2, 8).permute(0, 1, 3, 2, 4) \
        .contiguous().view(n, k)


def quantize_fp8_weight(w: torch.Tensor):
    """Per-output-row fp8 e4m3 weight quantization in the kernel's
    pair-swizzled layout: returns (w8 uint8 [N,K], w_scale f32 [N])."""
    amax = w.float().abs().amax(dim=1).clamp(min=1e-8)
    scale = amax / FP8_MAX
    q = (w.float() / scale[:, None]).to(torch.float8_e4m3fn)
    q8 = _fp8_pair_swizzle(q.view(torch.uint8))
    return q8.contiguous(), scale.to(torch.float32).contiguous()


def quant_fp8_rows(a: torch.Tensor, a8: torch.Tensor = None,
                   a_scale: torch.Tensor = None):
    """Dynamic per-row activation quantization to fp8 e4m3."""
    rows, cols = a.shape[0], a.shape[-1]
    if a.is_cuda:
        ops = _require_hip()
        if a8 is None:
            a8 = torch.empty(a.shape, dtype=torch.uint8, device=a.device)
        if a_scale is None:
            a_scale = torch.empty(rows, dtype=torch.float32,
                                  device=a.device)
        ops.quant_fp8_rows(a8, a_scale, a)
        return a8, a_scale
    amax = a.float().abs().amax(dim=-1).clamp(min=1e-8)
    scale = amax / FP8_MAX
    q = (a.float() / scale[:, None]).to(torch.float8_e4m3fn)
    q = _fp8_pair_swizzle(q.view(torch.uint8))
    if a8 is not None:
        a8.copy_(q)
        a_scale.copy_(scale)
        return a8, a_scale
    return q.contiguous(), scale.to(torch.float32).contiguous()


def skinny_gemm_fp8(a8: torch.Tensor, a_scale: torch.Tensor,
                    w8: torch.Tensor, w_scale: torch.Tensor,
                    out: torch.Tensor = None, c_f32: torch.Tensor = None,
                    ksplit: int = 1) -> torch.Tensor:
    """out[M,N] = (a8*a_scale[m]) @ (w8*w_scale[n])^T in bf16."""
    global _EMPTY_F32

    M, K = a8.shape
    N = w8.shape[0]
    if a8.is_cuda:
        ops = _require_hip()
        if out is None:
            out = torch.empty(M, N, dtype=torch.bfloat16,
                              device=a8.device)
        if ksplit > 1 and c_f32 is None:
            c_f32 = torch.empty(ksplit * M * N, dtype=torch.float32,
                                device=a8.device)
        if c_f32 is None:
            if _EMPTY_F32 is None or _EMPTY_F32.device != a8.device:
                _EMPTY_F32 = torch.empty(1, dtype=torch.float32,
                                         device=a8.device)
            c_f32 = _EMPTY_F32
        ops.skinny_gemm_fp8(out, c_f32, a8, a_scale, w8, w_scale, ksplit)
        return out
    a = _fp8_pair_unswizzle(a8).view(torch.float8_e4m3fn).float() * \
        a_scale[:, None].float()
    w = _fp8_pair_unswizzle(w8).view(torch.float8_e4m3fn).float() * \
        w_scale[:, None].float()
    result = (a @ w.t()).to(torch.bfloat16)
    if out is not None:
        out.copy_(result)
        return out
    return result


def rope_kv_fused(qkv: torch.Tensor, k_cache: torch.Tensor,
                  v_cache: torch.Tensor, positions: torch.Tensor,
                  cos_sin: torch.Tensor, hq: int,
                  k_scale: torch.Tensor = None,
                  v_scale: torch.Tensor = None):
    """Fused decode rope(q,k) + KV append from the fused qkv buffer
    [B, (hq+2*hkv)*d].  With k_scale/v_scale the caches are fp8
    (uint8 e4m3 + per-row f32 scales)."""
    B = qkv.shape[0]
    hkv, d = k_cache.shape[1], k_cache.shape[3]
    if qkv.is_cuda:
        _require_hip().rope_kv_fused(qkv, k_cache, v_cache, positions,
                                     cos_sin, hq, k_scale, v_scale)
        return
    q = qkv[:, :hq * d].view(B, hq, d)
    k = qkv[:, hq * d:(hq + hkv) * d].view(B, hkv, d)
    v = qkv[:, (hq + hkv) * d:(hq + 2 * hkv) * d].view(B, hkv, d)
    rope_inplace(q, positions, cos_sin)
    rope_inplace(k, positions, cos_sin)
    if k_scale is not None:
        for b in range(B):
            pos = int(positions[b])
            k8, ks = quantize_kv_rows(k[b])
            v8, vs = quantize_kv_rows(v[b])
            k_cache[b, :, pos] = k8
            v_cache[b, :, pos] = v8
            k_scale.view(B, hkv, -1)[b, :, pos] = ks
            v_scale.view(B, hkv, -1)[b, :, pos] = vs
        return
    kv_append(k_cache, v_cache, k, v, positions)


def quantize_kv_rows(x: torch.Tensor):
    """Per-row (last-dim) OCP e4m3 quantization -> (uint8, f32 scales).
    Matches the rope_kv_fused_q8 kernel: scale = amax/448."""
    amax = x.float().abs().amax(dim=-1, keepdim=True)
    scales = torch.where(amax > 0, amax / 448.0,
                         torch.ones_like(amax))
    q8 = (x.float() / scales).to(torch.float8_e4m3fn).view(torch.uint8)
    return q8, scales.squeeze(-1)


def dequantize_kv_rows(q8: torch.Tensor, scales: torch.Tensor,
                       dtype=torch.float32):
    """Inverse of quantize_kv_rows (reference/tests)."""
    x = q8.view(torch.float8_e4m3fn).float()
    return (x * scales.unsqueeze(-1)).to(dtype)


# ------------------------------------------------------------- attention


def pick_attn_nsplit(B: int, Hkv: int, target: int = 2048,
                     seq_len: int = None) -> int:
    """Split-S factor for decode attention.  Measured (scripts/
    bench_attn_longctx.py, 32-row LDS chunks): ~2048 workgroups is the
    sweet spot — ns8 at B=32 ties ns4 on the S=160 headline and wins
    8-14% for S>=1024; the seq_len hint additionally keeps each
    split's chunk <= ~128 tokens for very long contexts."""
    base = max(B * Hkv, 1)
    fill = (target + base - 1) // base
    chunk = (seq_len + 127) // 128 if seq_len else 1
    n = max(1, fill, chunk)
    # round up to a power of two (combine kernel indexes splits evenly)
    n = 1 << (n - 1).bit_length()
    return min(n, 16)


def attn_decode(q: torch.Tensor, k_cache: torch.Tensor,
                v_cache: torch.Tensor, seq_lens: torch.Tensor,
                scale: float = None,
                out: torch.Tensor = None,
                partial_ws: torch.Tensor = None,
                nsplit: int = None,
                k_scale: torch.Tensor = None,
                v_scale: torch.Tensor = None) -> torch.Tensor:
    """GQA decode attention (flash-decode split-S on GPU).
    q [B,Hq,D], caches [B,Hkv,Smax,D] bf16 — or uint8 e4m3 with
    per-row k_scale/v_scale [B,Hkv,Smax] (fp8 KV mode)."""
    B, Hq, D = q.shape
    Hkv = k_cache.shape[1]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    if q.is_cuda:
        ops = _require_hip()
        if out is None:
            out = torch.empty_like(q)
        if nsplit is None:
            nsplit = pick_attn_nsplit(B, Hkv)
        if nsplit > 1 and partial_ws is None:
            partial_ws = torch.empty(B * Hq * nsplit * (D + 2),
                                     dtype=torch.float32, device=q.device)
        ops.attn_decode(out, q, k_cache, v_cache, seq_lens, scale,
                        partial_ws, nsplit, k_scale, v_scale)
        return out
    # fp32 reference
    if out is None:
        out = torch.empty_like(q)
    if k_scale is not None:
        k_cache = dequantize_kv_rows(k_cache,
                                     k_scale.view(B, Hkv, -1))
        v_cache = dequantize_kv_rows(v_cache,
                                     v_scale.view(B, Hkv, -1))
    G = Hq // Hkv
    for b in range(B):
        length = int(seq_lens[b])
        for h in range(Hq):
            kvh = h // G
            qv = q[b, h].float()
            keys = k_cache[b, kvh, :length].float()
            vals = v_cache[b, kvh, :length].float()
            scores = torch.softmax(keys @ qv * scale, dim=0)
            out[b, h] = (scores @ vals).to(q.dtype)
    return out


# -------------------------------------------------------- packed prefill


def rope_kv_varlen(qkv: torch.Tensor, k_cache: torch.Tensor,
                   v_cache: torch.Tensor, positions: torch.Tensor,
                   tok_slot: torch.Tensor, cos_sin: torch.Tensor, hq: int):
    """Packed-prefill rope(q,k) + KV append.  qkv [T, (hq+2*hkv)*d] is
    the packed projection buffer of several sequences; token t is roped
    in place at positions[t] and its k/v land in
    cache[tok_slot[t], :, positions[t]].  bf16 caches only."""
    T = qkv.shape[0]
    hkv, d = k_cache.shape[1], k_cache.shape[3]
    if qkv.is_cuda:
        _require_hip().rope_kv_varlen(qkv, k_cache, v_cache, positions,
                                      tok_slot, cos_sin, hq)
        return
    q = qkv[:, :hq * d].view(T, hq, d)
    k = qkv[:, hq * d:(hq + hkv) * d].view(T, hkv, d)
    v = qkv[:, (hq + hkv) * d:(hq + 2 * hkv) * d].view(T, hkv, d)
    rope_inplace(q, positions, cos_sin)
    rope_inplace(k, positions, cos_sin)
    for t in range(T):
        slot, pos = int(tok_slot[t]), int(positions[t])
        k_cache[slot, :, pos] = k[t]
        v_cache[slot, :, pos] = v[t]


def attn_prefill(q: torch.Tensor, k_cache: torch.Tensor,
                 v_cache: torch.Tensor, cu_seqlens: torch.Tensor,
                 slots: torch.Tensor, kv_start: torch.Tensor,
                 scale: float = None, out: torch.Tensor = None,
                 max_q_len: int = None) -> torch.Tensor:
    """Packed (varlen) causal GQA prefill attention over the KV cache.

    q [T, Hq, D] holds n sequences back to back: sequence i owns rows
    cu_seqlens[i]..cu_seqlens[i+1].  Its query j sits at position
    p = kv_start[i] + j and attends to rows 0..p of
    cache[slots[i], h // G] — the chunk's own k/v must already be in
    the cache (rope_kv_varlen).  Returns out [T, Hq*D] bf16.
    max_q_len (the longest chunk) sizes the GPU grid; pass it from the
    host-side lengths to avoid a device sync."""
    T, Hq, D = q.shape
    Hkv = k_cache.shape[1]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    if out is None:
        out = torch.empty(T, Hq * D, dtype=q.dtype, device=q.device)
    if q.is_cuda:
        ops = _require_hip()
        if max_q_len is None:
            cu = cu_seqlens.tolist()
            max_q_len = max((b - a for a, b in zip(cu, cu[1:])), default=0)
        ops.attn_prefill(out, q, k_cache, v_cache, cu_seqlens, slots,
                         kv_start, scale, int(max_q_len))
        return out
    # fp32 reference: one query row at a time, the same expressions as
    # the attn_decode reference (so a length-1 chunk matches it bit
    # for bit)
    G = Hq // Hkv
    cu = cu_seqlens.tolist()
    out_v = out.view(T, Hq, D)
    for i in range(len(cu) - 1):
        slot, start = int(slots[i]), int(kv_start[i])
        for j in range(cu[i + 1] - cu[i]):
            row = cu[i] + j
            length = start + j + 1
            for h in range(Hq):
                kvh = h // G
                qv = q[row, h].float()
                keys = k_cache[slot, kvh, :length].float()
                vals = v_cache[slot, kvh, :length].float()
                scores = torch.softmax(keys @ qv * scale, dim=0)
                out_v[row, h] = (scores @ vals).to(q.dtype)
    return out


# ---------------------------------------------------------- prefix cache

KV_BLOCK_TOKENS = 32    # rows of one prefix-cache block


def kv_block_copy(src_k: torch.Tensor, src_v: torch.Tensor,
                  dst_k: torch.Tensor, dst_v: torch.Tensor,
                  src_row: torch.Tensor, src_blk: torch.Tensor,
                  dst_row: torch.Tensor, dst_blk: torch.Tensor):
    """Copy 32-token KV blocks between two bf16 tensors
    src [L, Rs, Hkv, Ss, D] and dst [L, Rd, Hkv, Sd, D]: entry i moves
    rows [src_blk[i]*32, +32) of src[:, src_row[i]] to rows
    [dst_blk[i]*32, +32) of dst[:, dst_row[i]], for every layer and KV
    head, K and V, in ONE launch.  The prefix-cache pool is
    [L, N, Hkv, 32, D] (block index 0) and the engine cache
    [L, B, Hkv, Smax, D], so the same op gathers pool -> slot and
    scatters slot -> pool.  The four index vectors are int32 [n].  An
    entry whose row is out of range, or whose block would reach past Ss
    or Sd, is skipped as a whole.  The caller keeps destinations
    distinct."""
    tensors = (("src_k", src_k), ("src_v", src_v),
               ("dst_k", dst_k), ("dst_v", dst_v))
    indices = (("src_row", src_row), ("src_blk", src_blk),
               ("dst_row", dst_row), ("dst_blk", dst_blk))
    device = src_k.device
    for name, t in tensors:
        if t.dtype != torch.bfloat16:
            raise ValueError(f"{name} must be bf16, got {t.dtype}")
        if t.dim() != 5:
            raise ValueError(f"{name} must be [L, R, Hkv, S, D], got "
                             f"{t.dim()} dimensions")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if t.device != device:
            raise ValueError(f"{name} is on {t.device}, src_k on {device}")
    if src_v.shape != src_k.shape or dst_v.shape != dst_k.shape:
        raise ValueError("K and V must have equal shapes: src "
                         f"{tuple(src_k.shape)}/{tuple(src_v.shape)}, dst "
                         f"{tuple(dst_k.shape)}/{tuple(dst_v.shape)}")
    L, Rs, Hkv, Ss, D = src_k.shape
    Rd, Sd = dst_k.shape[1], dst_k.shape[3]
    if (dst_k.shape[0], dst_k.shape[2], dst_k.shape[4]) != (L, Hkv, D):
        raise ValueError(f"src {tuple(src_k.shape)} and dst "
                         f"{tuple(dst_k.shape)} differ in L, Hkv or D")
    if (D * 2) % 16 != 0:
        raise ValueError(f"head dim {D}: rows must be a multiple of 16 "
                         "bytes")
    n = src_row.numel()
    for name, t in indices:
        if t.dtype != torch.int32 or t.dim() != 1:
            raise ValueError(f"{name} must be a 1-d int32 tensor")
        if t.device != device:
            raise ValueError(f"{name} is on {t.device}, src_k on {device}")
        if t.numel() != n:
            raise ValueError(f"{name} has {t.numel()} entries, src_row "
                             f"{n}")
    if n == 0:
        return
    if src_k.is_cuda:
        _require_hip().kv_block_copy(
            src_k, src_v, dst_k, dst_v, src_row.contiguous(),
            src_blk.contiguous(), dst_row.contiguous(),
            dst_blk.contiguous())
        return
    BT = KV_BLOCK_TOKENS
    for sr, sb, dr, db in zip(src_row.tolist(), src_blk.tolist(),
                              dst_row.tolist(), dst_blk.tolist()):
        if not (0 <= sr < Rs and 0 <= dr < Rd and sb >= 0 and db >= 0
                and (sb + 1) * BT <= Ss and (db + 1) * BT <= Sd):
            continue
        dst_k[:, dr, :, db * BT:(db + 1) * BT] = \
            src_k[:, sr, :, sb * BT:(sb + 1) * BT]
        dst_v[:, dr, :, db * BT:(db + 1) * BT] = \
            src_v[:, sr, :, sb * BT:(sb + 1) * BT]


# -------------------------------------------------- speculative decoding

VERIFY_MAX_QL = 8       # query rows per sequence in one verify pass
_VERIFY_WS_ROW = 128 + 4  # f32 per (row, head, split): o[128], m, l, pad


def pick_verify_nsplit(B: int, Hkv: int, Smax: int,
                       target: int = 512) -> int:
    """Split-S factor for attn_verify.  Measured (scripts/
    bench_verify.py, B=32, Hkv=8, QL=4): the ~2048 workgroups that suit
    attn_decode are too many here — a workgroup streams a whole KV head
    for G x QL columns, two of them fit a CU, and every extra split
    costs G x QL partial rows of workspace traffic.  Context 1024:
    ns1 28.8, ns2 28.1, ns4 32.7, ns8 37.4, ns16 50.5 us; context 4096:
    104.5, 98.6, 101.5, 110.8, 125.2 us.  So aim at ~512 workgroups,
    capped at 16 and at the 64-key tiles of the cache."""
    base = max(B * Hkv, 1)
    n = max(1, target // base)
    n = 1 << (n.bit_length() - 1)  # round down to a power of two
    return max(1, min(n, 16, (Smax + 63) // 64))


def attn_verify_ws_numel(B: int, QL: int, Hq: int, nsplit: int) -> int:
    """f32 elements of the split-S workspace ``attn_verify`` needs."""
    return B * QL * Hq * nsplit * _VERIFY_WS_ROW


def attn_verify(q: torch.Tensor, k_cache: torch.Tensor,
                v_cache: torch.Tensor, base_lens: torch.Tensor,
                scale: float = None, out: torch.Tensor = None,
                nsplit: int = None,
                partial_ws: torch.Tensor = None) -> torch.Tensor:
    """Speculative-verify GQA attention: a handful of query rows per
    sequence against a long cached prefix.

    q [B, QL, Hq, D] bf16 (may be a strided view into the fused qkv
    buffer), caches [B, Hkv, Smax, D] bf16, base_lens [B] int32 = rows
    cached BEFORE these QL tokens.  Query j of row b sits at position
    base_lens[b] + j and attends to rows 0..base_lens[b]+j of
    cache[b, h // G]; the QL new k/v rows must already be in the cache
    (rope_kv_varlen).  Returns out [B*QL, Hq*D] bf16.

    D = 128, G <= 8, 1 <= QL <= 8, bf16 caches — anything else raises
    ValueError.  On GPU one workgroup serves a whole KV head (K/V read
    once for its G q-heads) and the context is split nsplit ways
    (default: pick_verify_nsplit);
    pass out/partial_ws (attn_verify_ws_numel) to avoid allocation."""
    if q.dim() != 4 or k_cache.dim() != 4:
        raise ValueError("attn_verify: q must be [B, QL, Hq, D] and the "
                         "caches [B, Hkv, Smax, D]")
    B, QL, Hq, D = q.shape
    Hkv, Smax = k_cache.shape[1], k_cache.shape[2]
    if D != 128 or k_cache.shape[3] != D:
        raise ValueError(f"attn_verify needs head_dim 128, got {D}")
    if not 1 <= QL <= VERIFY_MAX_QL:
        raise ValueError(
            f"attn_verify needs 1 <= QL <= {VERIFY_MAX_QL}, got {QL}")
    if Hkv < 1 or Hq % Hkv or Hq // Hkv > 8:
        raise ValueError("attn_verify: q heads per kv head must divide "
                         f"and be <= 8 (Hq={Hq}, Hkv={Hkv})")
    if k_cache.dtype != torch.bfloat16 or v_cache.dtype != torch.bfloat16 \
            or q.dtype != torch.bfloat16:
        raise ValueError("attn_verify reads bf16 q and bf16 KV caches only")
    if k_cache.shape[0] != B or base_lens.numel() != B:
        raise ValueError("attn_verify: q, caches and base_lens must agree "
                         "on the batch size")
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    if out is None:
        out = torch.empty(B * QL, Hq * D, dtype=q.dtype, device=q.device)
    if q.is_cuda:
        ops = _require_hip()
        if nsplit is None:
            nsplit = pick_verify_nsplit(B, Hkv, Smax)
        nsplit = max(int(nsplit), 1)
        if nsplit > 1 and partial_ws is None:
            partial_ws = torch.empty(
                attn_verify_ws_numel(B, QL, Hq, nsplit),
                dtype=torch.float32, device=q.device)
        ops.attn_verify(out, q, k_cache, v_cache, base_lens, scale,
                        partial_ws, nsplit)
        return out
    # fp32 reference: the attn_prefill reference with every sequence a
    # chunk of QL rows on its own cache row
    cu = torch.arange(B + 1, dtype=torch.int32) * QL
    slots = torch.arange(B, dtype=torch.int32)
    return attn_prefill(q.reshape(B * QL, Hq, D), k_cache, v_cache, cu,
                        slots, base_lens, scale, out=out)


def ngram_draft(history: torch.Tensor, hist_lens: torch.Tensor, k: int,
                n: int = 2, out: torch.Tensor = None) -> torch.Tensor:
    """Prompt-lookup drafter: propose k tokens per row from the row's
    own history [B, L] int64 (hist_lens [B] int32 valid tokens each).

    With len = hist_lens[b] clamped to [0, L]: find the LARGEST p with
    p + n < len and history[b, p:p+n] == history[b, len-n:len]; then
    drafts[b, j] = history[b, p+n+j] while p+n+j < len.  Every other
    draft — also when nothing matches or len < n+1 — is the last token
    history[b, len-1]; len == 0 gives zeros.  Runs on the device
    without a host round trip; returns drafts [B, k] int64."""
    if history.dim() != 2 or history.dtype != torch.int64:
        raise ValueError("ngram_draft: history must be [B, L] int64")
    k, n = int(k), int(n)
    if k < 1 or not 1 <= n <= 64:
        raise ValueError("ngram_draft needs k >= 1 and 1 <= n <= 64")
    B, L = history.shape
    if hist_lens.numel() != B:
        raise ValueError("ngram_draft: one hist_lens entry per row")
    if out is None:
        out = torch.empty(B, k, dtype=torch.int64, device=history.device)
    if history.is_cuda:
        _require_hip().ngram_draft(out, history, hist_lens, n)
        return out
    lens = hist_lens.tolist()
    for b in range(B):
        length = max(0, min(int(lens[b]), L))
        if length == 0:
            out[b] = 0
            continue
        row = history[b, :length].tolist()
        tail = row[length - n:]
        match = -1
        if length >= n + 1:
            for p in range(length - n - 1, -1, -1):
                if row[p:p + n] == tail:
                    match = p
                    break
        for j in range(k):
            src = match + n + j if match >= 0 else length
            out[b, j] = row[src] if src < length else row[-1]
    return out


# ------------------------------------------------------------ multi-LoRA

LORA_RANKS = (8, 16, 32, 64)   # table ranks the kernels are built for
LORA_MAX_ROWS = 64             # decode rows per launch


def _check_lora(rows, t, table, idx, width_name):
    """Shared argument checks of lora_shrink / lora_expand: rows is the
    bf16 [B, width] activation (x or y), table the [NA, ., .] bf16
    adapter table, t the f32 [B, R] intermediate."""
    for name, tensor, dtype in (("rows", rows, torch.bfloat16),
                                ("table", table, torch.bfloat16),
                                ("t", t, torch.float32),
                                ("idx", idx, torch.int32)):
        if tensor.dtype != dtype:
            raise ValueError(f"lora: {name} must be {dtype}, got "
                             f"{tensor.dtype}")
        if not tensor.is_contiguous():
            raise ValueError(f"lora: {name} must be contiguous")
    if rows.dim() != 2 or t.dim() != 2 or table.dim() != 3 or \
            idx.dim() != 1:
        raise ValueError("lora: expected rows [B, width], t [B, R], a "
                         "3-d table and idx [B]")
    B, width = rows.shape
    R = t.shape[1]
    if B > LORA_MAX_ROWS:
        raise ValueError(f"lora: B must be <= {LORA_MAX_ROWS}, got {B}")
    if t.shape[0] != B or idx.numel() != B:
        raise ValueError("lora: rows, t and idx must agree on B")
    if R not in LORA_RANKS:
        raise ValueError(f"lora: R must be one of {LORA_RANKS}, got {R}")
    if width % 8:
        raise ValueError(f"lora: {width_name} must be a multiple of 8, "
                         f"got {width}")


def lora_shrink(x: torch.Tensor, A: torch.Tensor, idx: torch.Tensor,
                out: torch.Tensor = None) -> torch.Tensor:
    """Multi-LoRA shrink for a decode batch: row b uses adapter idx[b],
    t[b, j] = sum_k x[b, k] * A[idx[b], j, k] with f32 accumulation.

    x [B, K] bf16 (B <= 64, K % 8 == 0), A [NA, R, K] bf16 with R in
    {8, 16, 32, 64}, idx [B] int32.  Returns t [B, R] f32 (``out`` when
    given).  Rows whose id is outside [0, NA) are skipped: their t row
    is left as it was.  Bad shapes, dtypes or layouts raise ValueError."""
    if A.dim() != 3:
        raise ValueError("lora_shrink: A must be [NA, R, K]")
    if out is None:
        out = torch.zeros(x.shape[0], A.shape[1], dtype=torch.float32,
                          device=x.device)
    _check_lora(x, out, A, idx, "K")
    if A.shape[1] != out.shape[1] or A.shape[2] != x.shape[1]:
        raise ValueError("lora_shrink: A must be [NA, R, K] matching "
                         "x [B, K] and t [B, R]")
    if x.is_cuda:
        _require_hip().lora_shrink(out, x, A, idx)
        return out
    NA = A.shape[0]
    for b, a in enumerate(idx.tolist()):
        if 0 <= a < NA:
            out[b] = A[a].float() @ x[b].float()
    return out


def lora_expand(y: torch.Tensor, t: torch.Tensor, Bm: torch.Tensor,
                idx: torch.Tensor) -> torch.Tensor:
    """Multi-LoRA expand, in place: y[b, n] = bf16(float(y[b, n]) +
    sum_j t[b, j] * Bm[idx[b], n, j]) — f32 accumulation, one rounding.

    y [B, N] bf16 (B <= 64, N % 8 == 0), t [B, R] f32, Bm [NA, N, R]
    bf16 (alpha / r already folded in), idx [B] int32.  Rows whose id
    is outside [0, NA) are left untouched.  Returns y."""
    if Bm.dim() != 3:
        raise ValueError("lora_expand: Bm must be [NA, N, R]")
    _check_lora(y, t, Bm, idx, "N")
    if Bm.shape[1] != y.shape[1] or Bm.shape[2] != t.shape[1]:
        raise ValueError("lora_expand: Bm must be [NA, N, R] matching "
                         "y [B, N] and t [B, R]")
    if y.is_cuda:
        _require_hip().lora_expand(y, t, Bm, idx)
        return y
    NA = Bm.shape[0]
    for b, a in enumerate(idx.tolist()):
        if 0 <= a < NA:
            y[b] = (y[b].float() + Bm[a].float() @ t[b]).to(y.dtype)
    return y


# ---------------------------------------------------------------- sampler

SAMPLE_MAX_ROWS = 64           # logits rows per launch
_PHILOX_M = (0xD2511F53, 0xCD9E8D57)   # round multipliers
_PHILOX_W = (0x9E3779B9, 0xBB67AE85)   # key increments


def philox4x32(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11) on numpy arrays: ``counter``
    is four and ``key`` two broadcastable arrays of 32-bit words; returns
    the output blocks as uint32 [..., 4]."""
    import numpy as np

    u64 = np.uint64
    mask, shift = u64(0xFFFFFFFF), u64(32)
    c = [np.asarray(word).astype(u64) for word in counter]
    k = [np.asarray(word).astype(u64) for word in key]
    for _ in range(10):
        p0 = u64(_PHILOX_M[0]) * c[0]
        p1 = u64(_PHILOX_M[1]) * c[2]
        c = [(p1 >> shift) ^ c[1] ^ k[0], p1 & mask,
             (p0 >> shift) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + u64(_PHILOX_W[0])) & mask,
             (k[1] + u64(_PHILOX_W[1])) & mask]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def sample_tokens_reference(logits, pos, temperature, top_k, top_p, min_p,
                            seed) -> dict:
    """The sampler's semantics, vectorised over rows in numpy; this is
    what ``sample_tokens`` computes for CPU tensors and what the kernel
    is tested against.  Takes the arguments of ``sample_tokens`` (any
    device) and returns numpy arrays: ``tokens`` int64, ``logprob`` f32
    and ``kept`` int32 per row, plus the intermediates a test needs to
    judge near-ties: ``s`` and ``u`` [B, V] f32, ``keep`` [B, V] bool,
    ``q`` [B, V] and ``Q``, ``need`` [B] uint64 and, for the top_p cut,
    ``tail_cut`` / ``tail_above`` [B] uint64 (the tail mass at the
    threshold value and at the next larger distinct value).  Rows with
    ``pos < 0`` are computed like the others; the caller skips them.

    Per row, z_i = float(logits[i]):
    - temperature == 0: argmax z, lowest index on ties, kept = 1.  The
      same holds for any temperature at which zmax / T (f32) is not the
      finite quotient of a positive T: negative, NaN, or so small that
      the division overflows.  No score can then be NaN or +inf.
    - otherwise s_i = z_i / T (f32), m = max s, e_i = expf(s_i - m),
      q_i = floor(e_i * 2^32 + 0.5) (u64, exact in f64), Q = sum q_i.
      A token is kept if it passes every active filter, each a threshold
      on the logit value (equal logits stay together):
      top_k (0 < k < V): z_i >= the k-th largest value;
      top_p (p < 1): z_i >= v*, the largest value whose tail mass
      sum_{z_j >= v*} q_j reaches need = ceil(f64(p) * f64(Q));
      min_p (> 0): f64(q_i) >= f64(min_p) * 2^32.
      need is at least 1 (top_p <= 0 keeps the maximum's tie group), and
      a row whose filters keep nothing (min_p > 1) falls back to the
      argmax with kept = 1: the token is always a valid index.
      The token is the argmax over kept i of s_i + g_i (lowest index on
      ties), g_i = -logf(-logf(u_i)), u_i = ((r_i >> 8) + 0.5) * 2^-24
      in f32 and at most 1 - 2^-24, r_i = word i & 3 of the Philox4x32-10
      block with counter (i >> 2, pos, 0, 0) and key (seed & 0xffffffff,
      seed >> 32).
    - logprob = (z_tok - zmax) - logf(sum expf(z_i - zmax)): the model's
      own distribution at T = 1, unfiltered."""
    import numpy as np

    f32, f64, u64 = np.float32, np.float64, np.uint64
    z = logits.detach().float().cpu().numpy()
    B, V = z.shape
    rows = np.arange(B)
    pos = pos.detach().cpu().numpy().astype(np.int64)
    T = temperature.detach().cpu().numpy().astype(f32)
    k = top_k.detach().cpu().numpy().astype(np.int64)
    p = top_p.detach().cpu().numpy().astype(f32)
    mp = min_p.detach().cpu().numpy().astype(f32)
    sd = seed.detach().cpu().numpy().astype(np.int64).astype(u64)
    zmax = z.max(axis=1)
    with np.errstate(all="ignore"):
        sampled = (T > 0) & np.isfinite(
            (zmax / np.where(T > 0, T, f32(1))).astype(f32))
    s = (z / np.where(sampled, T, f32(1))[:, None]).astype(f32)
    m = s.max(axis=1)
    e = np.exp((s - m[:, None]).astype(f32)).astype(f32)
    q = np.floor(e.astype(f64) * 4294967296.0 + 0.5).astype(u64)
    Q = q.sum(axis=1, dtype=u64)
    order = np.argsort(-z, axis=1, kind="stable")
    z_sorted = np.take_along_axis(z, order, axis=1)
    # top_k: the k-th largest value
    k_on = sampled & (k > 0) & (k < V)
    kth = z_sorted[rows, np.clip(k - 1, 0, V - 1)]
    keep = ~k_on[:, None] | (z >= kth[:, None])
    # top_p: first sorted index whose running mass reaches need; its
    # value is v* (its whole tie group ends at or after that index)
    p_on = sampled & (p < 1)
    need = np.maximum(np.ceil(np.where(p > 0, p, f32(0)).astype(f64)
                              * Q.astype(f64)), 1.0).astype(u64)
    cum = np.cumsum(np.take_along_axis(q, order, axis=1), axis=1, dtype=u64)
    cut = (cum >= need[:, None]).argmax(axis=1)
    v_star = z_sorted[rows, cut]
    keep &= ~p_on[:, None] | (z >= v_star[:, None])
    ge = z_sorted >= v_star[:, None]        # sorted: a prefix of each row
    gt = z_sorted > v_star[:, None]
    tail_cut = cum[rows, ge.sum(axis=1) - 1]
    n_gt = gt.sum(axis=1)
    tail_above = np.where(n_gt > 0, cum[rows, np.maximum(n_gt, 1) - 1],
                          u64(0)).astype(u64)
    # min_p
    mp_on = sampled & (mp > 0)
    keep &= ~mp_on[:, None] | (q.astype(f64) >=
                               mp.astype(f64)[:, None] * 4294967296.0)
    # counter-based noise: block c serves tokens 4c .. 4c + 3
    blocks = philox4x32(
        (np.arange(V // 4, dtype=u64)[None, :],
         (pos & 0xFFFFFFFF).astype(u64)[:, None], 0, 0),
        ((sd & u64(0xFFFFFFFF))[:, None], (sd >> u64(32))[:, None]))
    r = blocks.reshape(B, V)
    u = ((r >> np.uint32(8)).astype(f32) + f32(0.5)) * f32(2.0 ** -24)
    u = np.minimum(u, f32(1.0 - 2.0 ** -24)).astype(f32)
    g = (-np.log(-np.log(u))).astype(f32)
    drawn = sampled & keep.any(axis=1)      # nothing kept: the argmax
    score = np.where(keep, (s + g).astype(f32), f32(-np.inf))
    tokens = np.where(drawn, score.argmax(axis=1), z.argmax(axis=1))
    kept = np.where(drawn, keep.sum(axis=1), 1).astype(np.int32)
    lsum = np.exp((z - zmax[:, None]).astype(f32)).sum(axis=1, dtype=f32)
    logprob = ((z[rows, tokens] - zmax).astype(f32)
               - np.log(lsum).astype(f32)).astype(f32)
    return {"tokens": tokens.astype(np.int64), "logprob": logprob,
            "kept": kept, "s": s, "u": u, "keep": keep, "q": q, "Q": Q,
            "need": need, "tail_cut": tail_cut, "tail_above": tail_above}


def _check_sample(logits, per_row, out_tokens, out_logprob, out_kept):
    """Argument checks of sample_tokens; ValueError before any launch."""
    checks = [("logits", logits, torch.bfloat16)]
    checks += [(name, tensor, dtype) for name, (tensor, dtype)
               in per_row.items()]
    checks.append(("out_tokens", out_tokens, torch.int64))
    if out_logprob is not None:
        checks.append(("out_logprob", out_logprob, torch.float32))
    if out_kept is not None:
        checks.append(("out_kept", out_kept, torch.int32))
    for name, tensor, dtype in checks:
        if not isinstance(tensor, torch.Tensor):
            raise ValueError(f"sample_tokens: {name} must be a tensor")
        if tensor.dtype != dtype:
            raise ValueError(f"sample_tokens: {name} must be {dtype}, got "
                             f"{tensor.dtype}")
        if not tensor.is_contiguous():
            raise ValueError(f"sample_tokens: {name} must be contiguous")
        if tensor.device != logits.device:
            raise ValueError(f"sample_tokens: {name} is on {tensor.device}, "
                             f"logits on {logits.device}")
    if logits.dim() != 2:
        raise ValueError("sample_tokens: logits must be [B, V], got "
                         f"{tuple(logits.shape)}")
    B, V = logits.shape
    if B > SAMPLE_MAX_ROWS:
        raise ValueError(f"sample_tokens: B must be <= {SAMPLE_MAX_ROWS}, "
                         f"got {B}")
    if V == 0 or V % 8 or V >= 1 << 24:
        raise ValueError("sample_tokens: V must be a positive multiple of "
                         f"8 below 2^24, got {V}")
    for name, tensor, _ in checks[1:]:
        if tensor.dim() != 1 or tensor.numel() != B:
            raise ValueError(f"sample_tokens: {name} must be [{B}], got "
                             f"{tuple(tensor.shape)}")
    if logits.is_cuda and logits.data_ptr() % 16:
        raise ValueError("sample_tokens: logits must be 16-byte aligned "
                         "(a view at an offset that is no multiple of 8 "
                         "elements is not)")


def sample_tokens(logits: torch.Tensor, pos: torch.Tensor,
                  temperature: torch.Tensor, top_k: torch.Tensor,
                  top_p: torch.Tensor, min_p: torch.Tensor,
                  seed: torch.Tensor, out_tokens: torch.Tensor,
                  out_logprob: torch.Tensor = None,
                  out_kept: torch.Tensor = None) -> torch.Tensor:
    """Fused per-row sampler: temperature, top_k, top_p, min_p and a
    seeded Gumbel-max draw in one launch, with the chosen token's
    logprob.  Every parameter is a tensor on the logits' device, read
    at run time: no allocation, no sync, hipGraph-capture safe.

    logits [B, V] bf16 (B <= 64, V % 8 == 0); pos [B] int32 (the
    position of the token being generated: the noise counter);
    temperature / top_p / min_p [B] f32; top_k [B] int32; seed [B]
    int64; out_tokens [B] int64; out_logprob [B] f32 and out_kept [B]
    int32 optional.  temperature 0 = greedy, top_k 0 / top_p 1 /
    min_p 0 = filter off.  Rows with pos < 0 are skipped and leave all
    outputs untouched.  A row's result depends only on its own logits
    and parameters, never on B or on the other rows, and is bitwise
    reproducible.  The exact semantics: ``sample_tokens_reference``.
    Logits must be finite.  Parameters outside their ranges (temperature
    < 0, NaN or too small to divide by, top_p <= 0, min_p > 1) degrade
    to the argmax as the reference states, never to an invalid token.
    Bad shapes, dtypes or layouts, logits not 16-byte aligned on the
    GPU included, raise ValueError before any launch."""
    _check_sample(
        logits,
        {"pos": (pos, torch.int32), "temperature": (temperature,
                                                    torch.float32),
         "top_k": (top_k, torch.int32), "top_p": (top_p, torch.float32),
         "min_p": (min_p, torch.float32), "seed": (seed, torch.int64)},
        out_tokens, out_logprob, out_kept)
    if logits.is_cuda:
        _require_hip().sample_tokens(logits, pos, temperature, top_k, top_p,
                                     min_p, seed, out_tokens, out_logprob,
                                     out_kept)
        return out_tokens
    if logits.shape[0] == 0:
        return out_tokens
    ref = sample_tokens_reference(logits, pos, temperature, top_k, top_p,
                                  min_p, seed)
    live = pos >= 0
    out_tokens[live] = torch.from_numpy(ref["tokens"])[live]
    if out_logprob is not None:
        out_logprob[live] = torch.from_numpy(ref["logprob"])[live]
    if out_kept is not None:
        out_kept[live] = torch.from_numpy(ref["kept"])[live]
    return out_tokens


# ------------------------------------------------------ logit processors

LOGIT_BIAS_MAX = 64            # bias entries per row
LOGIT_TILE = 2048              # columns per workgroup of the kernel


def _check_logit_processors(logits, state, penalties, bias_ids, bias_val,
                            bias_n, tokens, rows):
    """Argument checks of logit_processors; ValueError before any
    launch."""
    checks = [("logits", logits, torch.bfloat16),
              ("state", state, torch.int32),
              ("penalties", penalties, torch.float32),
              ("bias_ids", bias_ids, torch.int32),
              ("bias_val", bias_val, torch.float32),
              ("bias_n", bias_n, torch.int32)]
    if tokens is not None:
        checks.append(("tokens", tokens, torch.int64))
    if rows is not None:
        checks.append(("rows", rows, torch.int32))
    for name, tensor, dtype in checks:
        if not isinstance(tensor, torch.Tensor):
            raise ValueError(f"logit_processors: {name} must be a tensor")
        if tensor.dtype != dtype:
            raise ValueError(f"logit_processors: {name} must be {dtype}, "
                             f"got {tensor.dtype}")
        if not tensor.is_contiguous():
            raise ValueError(f"logit_processors: {name} must be contiguous")
        if tensor.device != logits.device:
            raise ValueError(f"logit_processors: {name} is on "
                             f"{tensor.device}, logits on {logits.device}")
    if logits.dim() != 2:
        raise ValueError("logit_processors: logits must be [B, V], got "
                         f"{tuple(logits.shape)}")
    B, V = logits.shape
    if B > SAMPLE_MAX_ROWS:
        raise ValueError(f"logit_processors: B must be <= "
                         f"{SAMPLE_MAX_ROWS}, got {B}")
    if V == 0 or V % 8 or V >= 1 << 24:
        raise ValueError("logit_processors: logits [B, V] need V a positive "
                         f"multiple of 8 below 2^24, got {V}")
    if state.dim() != 2 or state.shape[1] != V:
        raise ValueError(f"logit_processors: state must be [S, {V}], got "
                         f"{tuple(state.shape)}")
    shapes = [("penalties", penalties, (B, 3)),
              ("bias_ids", bias_ids, (B, LOGIT_BIAS_MAX)),
              ("bias_val", bias_val, (B, LOGIT_BIAS_MAX)),
              ("bias_n", bias_n, (B,))]
    if tokens is not None:
        shapes.append(("tokens", tokens, (B,)))
    if rows is not None:
        shapes.append(("rows", rows, (B,)))
    for name, tensor, shape in shapes:
        if tuple(tensor.shape) != shape:
            raise ValueError(f"logit_processors: {name} must be "
                             f"{list(shape)}, got {tuple(tensor.shape)}")
    if logits.is_cuda and (logits.data_ptr() % 16 or state.data_ptr() % 16):
        raise ValueError("logit_processors: logits and state must be "
                         "16-byte aligned (a view at an offset that is no "
                         "multiple of 8 / 4 elements is not)")


def logit_processors(logits: torch.Tensor, state: torch.Tensor,
                     penalties: torch.Tensor, bias_ids: torch.Tensor,
                     bias_val: torch.Tensor, bias_n: torch.Tensor,
                     tokens: torch.Tensor = None,
                     rows: torch.Tensor = None) -> torch.Tensor:
    """Repetition, presence and frequency penalties and a logit bias,
    applied in place to the logits a sampler reads next, from a token-
    state table that the same call maintains.  Every parameter is a
    tensor on the logits' device, read at run time: no allocation, no
    sync, hipGraph-capture safe.

    logits [B, V] bf16 (B <= 64, V % 8 == 0); state [S, V] int32 with
    ``state[r, v] = 2 * n_out + in_prompt`` (how often sequence r has
    generated token v, and whether its prompt holds it); penalties
    [B, 3] f32, columns repetition r, presence p, frequency f; bias_ids
    [B, 64] int32 and bias_val [B, 64] f32, of which the first
    ``bias_n[b]`` (int32, clamped to [0, 64]) are live and an id outside
    [0, V) is ignored; tokens [B] int64 or None, each row's pending
    token (generated, not yet counted); rows [B] int32 or None, the
    state row of logits row b (None: b).

    A row with r == 1, p == 0, f == 0 and no live bias is neutral.  A
    neutral row and a row whose state row is outside [0, S) are skipped
    whole: logits and state untouched, the pending token not counted.
    For every other row, in this order:
    1. a pending token t in [0, V) is counted, state[row, t] += 2 (any
       other t is ignored), before column t is evaluated;
    2. per column v, c = state[row, v], n = c >> 1, z = float(logit):
       c != 0 and r != 1: z = z / r if z > 0 else z * r
       n > 0:             z = (z - f * float(n)) - p
       v a live id:       z = z + bias_val
       and the logit becomes bf16(z), rounded to nearest even.
    Every step is one separately rounded f32 operation; this CPU branch
    (torch elementwise ops) is the reference the kernel matches bit for
    bit.  Two logits rows naming one state row are forbidden; of
    duplicate live ids one value applies, unspecified which.  Bad
    shapes, dtypes, layouts or devices raise ValueError before any
    launch."""
    _check_logit_processors(logits, state, penalties, bias_ids, bias_val,
                            bias_n, tokens, rows)
    if logits.is_cuda:
        _require_hip().logit_processors(logits, state, penalties, bias_ids,
                                        bias_val, bias_n, tokens, rows)
        return logits
    B, V = logits.shape
    S = state.shape[0]
    for b in range(B):
        row = b if rows is None else int(rows[b])
        rep, pres, freq = penalties[b]          # 0-dim f32 tensors
        live = min(max(int(bias_n[b]), 0), LOGIT_BIAS_MAX)
        if not 0 <= row < S:
            continue
        if rep == 1 and pres == 0 and freq == 0 and live == 0:
            continue
        counts = state[row]
        if tokens is not None and 0 <= int(tokens[b]) < V:
            counts[int(tokens[b])] += 2
        z = logits[b].float()
        if rep != 1:
            z = torch.where((counts != 0) & (z > 0), z / rep,
                            torch.where(counts != 0, z * rep, z))
        n = counts >> 1
        z = torch.where(n > 0, (z - freq * n.float()) - pres, z)
        ids = bias_ids[b, :live].long()
        inside = (ids >= 0) & (ids < V)
        ids = ids[inside]
        z[ids] = z[ids] + bias_val[b, :live][inside]
        logits[b] = z.to(torch.bfloat16)
    return logits


def kv_append(k_cache, v_cache, k_new, v_new, positions):
    """Scatter the new token K/V into the cache at positions[b]."""
    if k_cache.is_cuda:
        _require_hip().kv_append(k_cache, v_cache, k_new, v_new, positions)
        return
    B = k_cache.shape[0]
    for b in range(B):
        pos = int(positions[b])
        k_cache[b, :, pos] = k_new[b]
        v_cache[b, :, pos] = v_new[b]


# ---------------------------------------------------------------- others


def softmax(x: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    if x.is_cuda:
        ops = _require_hip()
        if out is None:
            out = torch.empty_like(x)
        ops.softmax(out, x)
        return out
    result = torch.softmax(x.float(), dim=-1).to(x.dtype)
    if out is not None:
        out.copy_(result)
        return out
    return result


def tree_ensemble_predict(features: torch.Tensor, nodes: dict,
                          base_score: float = 0.0,
                          out: torch.Tensor = None) -> torch.Tensor:
    """GBDT margin prediction.  nodes: dict of flat SoA int32/f32
    tensors (feature_idx/threshold/left/right/leaf_value/tree_offsets),
    on the same device as features."""
    if features.is_cuda:
        ops = _require_hip()
        if out is None:
            out = torch.empty(features.shape[0], dtype=torch.float32,
                              device=features.device)
        ops.tree_ensemble(out, features, nodes["feature_idx"],
                          nodes["threshold"], nodes["left"], nodes["right"],
                          nodes["leaf_value"], nodes["tree_offsets"],
                          base_score)
        return out
    # reference: walk trees in python
    n = features.shape[0]
    result = torch.full((n,), base_score, dtype=torch.float32)
    fidx = nodes["feature_idx"].tolist()
    thr = nodes["threshold"].tolist()
    left = nodes["left"].tolist()
    right = nodes["right"].tolist()
    leaf = nodes["leaf_value"].tolist()
    offsets = nodes["tree_offsets"].tolist()
    feats = features.tolist()
    for i in range(n):
        score = base_score
        for t in range(len(offsets) - 1):
            node = offsets[t]
            while fidx[node] >= 0:
                node = left[node] if feats[i][fidx[node]] < thr[node] \
                    else right[node]
            score += leaf[node]
        result[i] = score
    if out is not None:
        out.copy_(result)
        return out
    return result


def window_ingest(ring, keys, values, period_idx):
    """Fold (sum, count) period cells.  An f64 ring accumulates the
    SQUARES of the values instead (the stdvar/stddev ring — f32
    sum-of-squares cancels catastrophically)."""
    if ring.is_cuda:
        _require_hip().window_ingest(ring, keys, values, period_idx)
        return ring
    import numpy as np

    n_periods = ring.shape[1]
    flat_idx = keys.numpy().astype(np.int64) * n_periods + \
        (period_idx.numpy().astype(np.int64) % n_periods)
    view = ring.numpy().reshape(-1, 4)
    vals = values.numpy()
    # sort + reduceat segment sums (np.add.at is per-element)
    order = np.argsort(flat_idx, kind="stable")
    flat_s = flat_idx[order]
    vals_s = vals[order]
    uniq, starts = np.unique(flat_s, return_index=True)
    ends = np.append(starts[1:], len(flat_s))
    counts = (ends - starts).astype(view.dtype)
    if ring.dtype == torch.float64:
        vals_s = vals_s.astype(np.float64)
        view[uniq, 0] += np.add.reduceat(vals_s * vals_s, starts)
        view[uniq, 1] += counts
        view[uniq, 2] += np.add.reduceat(vals_s, starts)  # f64 sum
        return ring
    view[uniq, 0] += np.add.reduceat(vals_s, starts)
    view[uniq, 1] += counts
    return ring


# ordered-f32 transform (monotone f32 -> u32 so integer min/max give
# float order) — numpy mirror of the kernel's f32_to_ordered
def _f32_to_ordered_np(values):
    import numpy as np

    bits = values.astype(np.float32).view(np.uint32)
    return np.where(bits & 0x80000000, ~bits, bits | 0x80000000)


def _ordered_to_f32_np(keys):
    import numpy as np

    keys = keys.astype(np.uint32)
    bits = np.where(keys & 0x80000000, keys & 0x7FFFFFFF, ~keys)
    return bits.astype(np.uint32).view(np.float32)


MM_MIN_EMPTY = -1          # int32 view of 0xFFFFFFFF
MM_MAX_EMPTY = 0
FL_FIRST_EMPTY = -1        # int64 view of 0xFFFFFFFFFFFFFFFF
FL_LAST_EMPTY = 0


def window_ingest_mm(ring_mm, keys, values, period_idx):
    """Fold per-period MIN/MAX cells (ring_mm int32 = ordered-f32
    bits; empty = MM_MIN_EMPTY/MM_MAX_EMPTY)."""
    if ring_mm.is_cuda:
        _require_hip().window_ingest_mm(ring_mm, keys, values, period_idx)
        return ring_mm
    import numpy as np

    n_periods = ring_mm.shape[1]
    flat = keys.numpy().astype(np.int64) * n_periods + \
        (period_idx.numpy().astype(np.int64) % n_periods)
    ov = _f32_to_ordered_np(values.numpy())
    view = ring_mm.numpy().view(np.uint32).reshape(-1, 2)
    # sort + reduceat: one segment min/max per touched cell (ufunc.at
    # is a per-element python-level loop — too slow for 1M-event
    # batches)
    order = np.argsort(flat, kind="stable")
    flat_s, ov_s = flat[order], ov[order]
    uniq, starts = np.unique(flat_s, return_index=True)
    seg_min = np.minimum.reduceat(ov_s, starts)
    seg_max = np.maximum.reduceat(ov_s, starts)
    view[uniq, 0] = np.minimum(view[uniq, 0], seg_min)
    view[uniq, 1] = np.maximum(view[uniq, 1], seg_max)
    return ring_mm


def window_ingest_fl(ring_fl, keys, values, timestamps, period_idx):
    """Fold per-period FIRST/LAST cells (ring_fl int64 packed
    (ts << 32) | ordered-f32; empty = FL_FIRST_EMPTY/FL_LAST_EMPTY)."""
    if ring_fl.is_cuda:
        _require_hip().window_ingest_fl(ring_fl, keys, values,
                                        timestamps, period_idx)
        return ring_fl
    import numpy as np

    n_periods = ring_fl.shape[1]
    flat = keys.numpy().astype(np.int64) * n_periods + \
        (period_idx.numpy().astype(np.int64) % n_periods)
    pack = (timestamps.numpy().astype(np.uint64) << np.uint64(32)) | \
        _f32_to_ordered_np(values.numpy()).astype(np.uint64)
    view = ring_fl.numpy().view(np.uint64).reshape(-1, 2)
    order = np.argsort(flat, kind="stable")
    flat_s, pack_s = flat[order], pack[order]
    uniq, starts = np.unique(flat_s, return_index=True)
    seg_min = np.minimum.reduceat(pack_s, starts)
    seg_max = np.maximum.reduceat(pack_s, starts)
    view[uniq, 0] = np.minimum(view[uniq, 0], seg_min)
    view[uniq, 1] = np.maximum(view[uniq, 1], seg_max)
    return ring_fl


def window_reduce_mmfl(ring_mm, ring_fl, window_periods: int,
                       current_period: int, out: torch.Tensor = None):
    """Reduce min/max/first/last over the covered window cells ->
    [keys, 4] f32 (min, max, first, last); empty windows yield 0 —
    callers mask by the count from window_reduce."""
    if ring_mm.is_cuda:
        ops = _require_hip()
        if out is None:
            out = torch.empty(ring_mm.shape[0], 4, dtype=torch.float32,
                              device=ring_mm.device)
        ops.window_reduce_mmfl(out, ring_mm, ring_fl, window_periods,
                               current_period)
        return out
    import numpy as np

    n_keys, n_periods, _ = ring_mm.shape
    cols = [(current_period - w) % n_periods
            for w in range(window_periods)]
    mm = ring_mm.numpy().view(np.uint32)
    fl = ring_fl.numpy().view(np.uint64)
    omin = mm[:, cols, 0].min(axis=1)
    omax = mm[:, cols, 1].max(axis=1)
    first_pack = fl[:, cols, 0].min(axis=1)
    last_pack = fl[:, cols, 1].max(axis=1)
    result = np.zeros((n_keys, 4), dtype=np.float32)
    has_min = omin != 0xFFFFFFFF
    has_max = omax != 0
    result[:, 0] = np.where(has_min, _ordered_to_f32_np(omin), 0.0)
    result[:, 1] = np.where(has_max, _ordered_to_f32_np(omax), 0.0)
    has_first = first_pack != np.uint64(0xFFFFFFFFFFFFFFFF)
    has_last = last_pack != 0
    result[:, 2] = np.where(
        has_first,
        _ordered_to_f32_np((first_pack & np.uint64(0xFFFFFFFF)
                            ).astype(np.uint32)), 0.0)
    result[:, 3] = np.where(
        has_last,
        _ordered_to_f32_np((last_pack & np.uint64(0xFFFFFFFF)
                            ).astype(np.uint32)), 0.0)
    tensor = torch.from_numpy(result)
    if out is not None:
        out.copy_(tensor)
        return out
    return tensor


def window_reduce(ring, window_periods: int, current_period: int,
                  out: torch.Tensor = None):
    if ring.is_cuda:
        ops = _require_hip()
        if out is None:
            out = torch.empty(ring.shape[0], 4, dtype=ring.dtype,
                              device=ring.device)
        ops.window_reduce(out, ring, window_periods, current_period)
        return out
    n_keys, n_periods, _ = ring.shape
    result = torch.zeros(n_keys, 4, dtype=ring.dtype)
    for w in range(window_periods):
        p = (current_period - w) % n_periods
        result[:, 0] += ring[:, p, 0]
        result[:, 1] += ring[:, p, 1]
        if ring.dtype == torch.float64:
            result[:, 2] += ring[:, p, 2]  # f64 sum slot
    if ring.dtype != torch.float64:
        counts = result[:, 1].clamp(min=1.0)
        result[:, 2] = result[:, 0] / counts
        result[:, 2] = torch.where(result[:, 1] > 0, result[:, 2],
                                   torch.zeros_like(result[:, 2]))
    if out is not None:
        out.copy_(result)
        return out
    return result
