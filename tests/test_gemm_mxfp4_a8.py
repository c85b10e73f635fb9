# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""The W4A8 mxfp4 GEMM, the natural-order activation quant and the
mxfp4a8 prefill mode without a GPU."""

import pytest
import torch

from mlrun_amd import ops
from mlrun_amd.models.llama import LlamaConfig, LlamaDecodeEngine, LlamaServer

from decode_refs import EPS32, R1, check, e4m3_decode, f64
from test_gemm_mxfp4 import BF16, dequant64, random_pack

U8 = torch.uint8


def test_natural_order_quant_is_the_unswizzled_default():
    a = (torch.randn(5, 320, generator=torch.Generator().manual_seed(1))
         * 3).to(BF16)
    swizzled, scale = ops.quant_fp8_rows(a)
    natural, scale_n = ops.quant_fp8_rows(a, swizzle=False)
    assert torch.equal(natural, ops._fp8_pair_unswizzle(swizzled))
    assert torch.equal(scale_n, scale)
    a8, a_scale = torch.empty(5, 320, dtype=U8), torch.empty(5)
    ops.quant_fp8_rows(a, a8, a_scale, swizzle=False)
    assert torch.equal(a8, natural) and torch.equal(a_scale, scale)


@pytest.mark.parametrize("m,n,k", [(65, 40, 640), (3, 7, 128)])
def test_cpu_gemm_against_float64(m, n, k):
    """Exact products, K fp32 additions and the row scale, one rounding."""
    w4, w_scale = random_pack(n, k, seed=k + m)
    g = torch.Generator().manual_seed(2)
    a8, a_scale = ops.quant_fp8_rows(
        (torch.randn(m, k, generator=g) * (1 + torch.arange(m))[:, None])
        .to(BF16), swizzle=False)
    a = e4m3_decode(a8) * f64(a_scale)[:, None]
    w = dequant64(w4, w_scale)
    ref = a @ w.t()
    bound = R1 * ref.abs() + (k + 3) * EPS32 * (a.abs() @ w.abs().t()) \
        * (1 + R1)
    out = torch.empty(m, n, dtype=BF16)
    assert ops.gemm_mxfp4_a8(a8, a_scale, w4, w_scale, out=out) is out
    check(out, ref, bound, f"cpu mxfp4a8 gemm m{m} n{n} k{k}")


@pytest.mark.parametrize("change", [
    dict(a8=torch.zeros(70, 256, dtype=BF16)),                # dtype
    dict(a8=torch.zeros(256, dtype=U8)),                      # rank
    dict(a8=torch.zeros(256, 70, dtype=U8).t()),              # contiguity
    dict(a8=torch.zeros(0, 256, dtype=U8),
         a_scale=torch.zeros(0)),                             # M < 1
    dict(a8=torch.zeros(70, 128, dtype=U8)),                  # K mismatch
    dict(a8=torch.zeros(70, 192, dtype=U8),
         w4=torch.zeros(8, 96, dtype=U8),
         w_scale=torch.zeros(8, 6, dtype=U8)),                # K % 128
    dict(a_scale=torch.zeros(69)),                            # scale length
    dict(a_scale=torch.zeros(70, dtype=torch.float64)),       # scale dtype
    dict(w_scale=torch.zeros(7, 8, dtype=U8)),                # N mismatch
    dict(w4=torch.zeros(8, 128, dtype=torch.int8)),           # dtype
    dict(out=torch.zeros(70, 9, dtype=BF16)),                 # out shape
    dict(out=torch.zeros(70, 8)),                             # out dtype
    dict(a8=torch.zeros(70, 256, dtype=U8, device="meta")),   # device
], ids=lambda c: "+".join(c))
def test_gemm_argument_errors(change):
    w4, w_scale = random_pack(8, 256, seed=3)
    args = dict(a8=torch.zeros(70, 256, dtype=U8), a_scale=torch.ones(70),
                w4=w4, w_scale=w_scale)
    with pytest.raises(ValueError):
        ops.gemm_mxfp4_a8(**{**args, **change})


def test_mode_errors_without_a_gpu():
    cfg = LlamaConfig.tiny(hidden_size=128, intermediate_size=256,
                           vocab_size=512)
    with pytest.raises(ValueError, match="mxfp4a8.*weight_dtype"):
        LlamaDecodeEngine(cfg, batch_size=2, device="cpu",
                          prefill_gemm="mxfp4a8")             # bf16 weights
    with pytest.raises(ValueError, match="mxfp4a8.*on cpu"):
        LlamaDecodeEngine(cfg, batch_size=2, device="cpu",
                          weight_dtype="mxfp4w", prefill_gemm="mxfp4a8")
    # release_masters goes with the mode: load() gets past that check and
    # fails where the engine finds no GPU
    server = LlamaServer(name="gen", config="tiny", batch_size=2,
                         device="cpu", weight_dtype="mxfp4w",
                         prefill_gemm="mxfp4a8", release_masters=True)
    with pytest.raises(ValueError, match="mxfp4a8.*on cpu"):
        server.load()
