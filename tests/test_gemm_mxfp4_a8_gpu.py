# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""The W4A8 mxfp4 tile GEMM (gemm_mxfp4_a8_tile_kernel) against float64,
and the mxfp4w engine that prefills with it."""

import functools

import pytest
import torch

from mlrun_amd import ops
from mlrun_amd.models.llama import LlamaConfig, LlamaDecodeEngine

from decode_refs import EPS32, MFMA_FP8_ACC, R1, check, e4m3_decode, f64
from test_gemm_mxfp4 import dequant64

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs MI355X")]
# the engine test's distance between "mxfp4a8" and "mxfp4" prefill logits,
# measured on MI355X (|logit| <= 0.86): pure e4m3 activation rounding
D_A8 = 0.0332


@functools.lru_cache(maxsize=None)
def gemm_case(m, n, k):
    """A real pack whose block scales differ per (row, block) by powers of
    two in 2^-3 .. 2^3, so a scale byte from the wrong row, block or step
    is off by 2x or more; activations with a per-row factor, quantized by
    the CPU branch.  Returns the operands, the float64 product of their
    exact values, and the bound: one bf16 rounding, K + 3 fp32 operations
    and the fp8 MFMA's accumulation term, as the fp8 GEMMs'."""
    g = torch.Generator().manual_seed(10 * k + m)
    spread = 2.0 ** torch.randint(-3, 4, (n, k // 32), generator=g)
    w4, w_scale = ops.quantize_mxfp4_weight(
        (torch.randn(n, k, generator=g) *
         spread.repeat_interleave(32, dim=1)).to(torch.bfloat16))
    step = 1.25 ** ((3 * torch.arange(m)) % 17).float()
    a8, a_scale = ops.quant_fp8_rows(
        (torch.randn(m, k, generator=g) * step[:, None]).to(torch.bfloat16),
        swizzle=False)
    a = e4m3_decode(a8) * f64(a_scale)[:, None]
    w = dequant64(w4, w_scale)
    ref = a @ w.t()
    bound = R1 * ref.abs() + ((k + 3) * EPS32 + MFMA_FP8_ACC) * \
        (a.abs() @ w.abs().t())
    return (a8, a_scale, w4, w_scale), ref, bound


def gemm(bn, a8, a_scale, w4, w_scale, out=None):
    """bn 0: the public op, which picks 64-wide tiles at shapes this
    small.  bn 128: the kernel's wide instance, through the binding."""
    if bn == 0:
        return ops.gemm_mxfp4_a8(a8, a_scale, w4, w_scale, out=out)
    if out is None:
        out = torch.empty(a8.shape[0], w4.shape[0], dtype=torch.bfloat16,
                          device=a8.device)
    ops._require_hip().gemm_mxfp4_a8_tile(out, a8, a_scale, w4, w_scale, bn)
    return out


# M: one clamped row, one or two M tiles, full and ragged; N: one clamped
# tile, an exact one, several with a ragged last; K: one step, tail-order
# scales only, one scale group plus a tail step, two groups plus a tail.
@pytest.mark.parametrize("bn", [0, 128])
@pytest.mark.parametrize("k", [128, 384, 640, 1152])
@pytest.mark.parametrize("n", [80, 128, 272])
@pytest.mark.parametrize("m", [1, 65, 128, 129, 200])
def test_kernel_against_float64(m, n, k, bn):
    case, ref, bound = gemm_case(m, n, k)
    got = gemm(bn, *(t.cuda() for t in case))
    check(got, ref, bound, f"mxfp4a8 tile gemm m{m} n{n} k{k} bn{bn}",
          kernel="gemm_mxfp4_a8_tile")


@pytest.mark.parametrize("bn", [0, 128])
def test_memory_past_the_operands_is_never_read(bn):
    """Each operand ends its buffer and NaN follows (e4m3 code 0x7F, fp4
    bytes under E8M0 NaN scales 0xFF, f32 NaN); out sits between sentinel
    rows, which stay."""
    m, n, k = 129, 80, 384
    case, ref, bound = gemm_case(m, n, k)

    def guarded(t, fill):
        buf = torch.full((2 * t.numel(),), fill, dtype=t.dtype, device="cuda")
        buf[:t.numel()] = t.flatten().cuda()
        return buf[:t.numel()].view(t.shape)

    operands = [guarded(t, fill) for t, fill in zip(
        case, (0x7F, float("nan"), 0xFF, 0xFF))]
    # 8 rows of n keep out 16-byte aligned
    frame = torch.full((m + 16, n), 77.0, dtype=torch.bfloat16, device="cuda")
    out = frame[8:8 + m]
    gemm(bn, *operands, out)
    assert (frame[:8] == 77.0).all() and (frame[8 + m:] == 77.0).all()
    check(out, ref, bound, f"mxfp4a8 tile gemm guarded bn{bn}")


def test_engine_prefills_on_the_packs_with_e4m3_activations():
    """X prefills 96 packed rows under "mxfp4a8", R under "mxfp4" on the
    same packs: the logits differ by the activations' e4m3 rounding alone,
    d_a8 (measured: D_A8 above; twice that is allowed, for other ROCm
    builds).  X is deterministic, leaves the slot state R leaves, and
    generates the same tokens once its masters are gone."""
    cfg = LlamaConfig.tiny(hidden_size=128, intermediate_size=256,
                           vocab_size=512)
    g = torch.Generator().manual_seed(8)
    prompts = [torch.randint(0, 512, (s,), generator=g).tolist()
               for s in (40, 31, 25)]
    x, r = (LlamaDecodeEngine(cfg, batch_size=3, device="cuda:0",
                              use_graph=False, seed=41,
                              weight_dtype="mxfp4w", prefill_gemm=mode)
            for mode in ("mxfp4a8", "mxfp4"))
    logits = x.prefill_packed(prompts, [0, 1, 2])
    assert torch.isfinite(logits).all()
    x.reset()
    assert torch.equal(x.prefill_packed(prompts, [0, 1, 2]), logits)
    ref = f64(r.prefill_packed(prompts, [0, 1, 2]))
    assert torch.equal(x.cache_lens, r.cache_lens)
    d_a8 = (f64(logits) - ref).abs().max().item()
    print(f"d_a8 {d_a8:.4g}  max |logit| {ref.abs().max().item():.3g}")
    assert 0 < d_a8 < 2 * D_A8

    prompt = torch.randint(0, 512, (3, 12), generator=g)
    x.reset()
    tokens = x.generate(prompt, max_new_tokens=4)
    x.release_master_weights()
    assert x.weights.lm_head is None
    x.reset()
    assert torch.equal(x.generate(prompt, max_new_tokens=4), tokens)
