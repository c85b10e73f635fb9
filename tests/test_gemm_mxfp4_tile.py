# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""The any-M mxfp4 GEMM and the mxfp4 prefill mode without a GPU."""

import pytest
import torch

from mlrun_amd import ops
from mlrun_amd.models.llama import LlamaConfig, LlamaDecodeEngine, LlamaServer

from decode_refs import EPS32, R1, check, f64
from test_gemm_mxfp4 import BF16, dequant64, random_pack


@pytest.mark.parametrize("m,n,k", [(65, 40, 640), (130, 7, 128)])
def test_cpu_gemm_against_float64(m, n, k):
    w4, w_scale = random_pack(n, k, seed=k + m)
    a = torch.randn(m, k, generator=torch.Generator().manual_seed(2)).to(BF16)
    w = dequant64(w4, w_scale)
    ref = f64(a) @ w.t()
    bound = R1 * ref.abs() + (k + 2) * EPS32 * (f64(a).abs() @ w.abs().t()) \
        * (1 + R1)
    out = torch.empty(m, n, dtype=BF16)
    assert ops.gemm_mxfp4(a, w4, w_scale, out=out) is out
    check(out, ref, bound, f"cpu mxfp4 gemm m{m} n{n} k{k}")


@pytest.mark.parametrize("change", [
    dict(a=torch.zeros(70, 256)),                             # dtype
    dict(a=torch.zeros(256, dtype=BF16)),                     # rank
    dict(a=torch.zeros(256, 70, dtype=BF16).t()),             # contiguity
    dict(a=torch.zeros(0, 256, dtype=BF16)),                  # M < 1
    dict(a=torch.zeros(70, 128, dtype=BF16)),                 # K mismatch
    dict(a=torch.zeros(70, 192, dtype=BF16),
         w4=torch.zeros(8, 96, dtype=torch.uint8),
         w_scale=torch.zeros(8, 6, dtype=torch.uint8)),       # K % 128
    dict(w_scale=torch.zeros(7, 8, dtype=torch.uint8)),       # N mismatch
    dict(w4=torch.zeros(8, 128, dtype=torch.int8)),           # dtype
    dict(out=torch.zeros(70, 9, dtype=BF16)),                 # out shape
    dict(out=torch.zeros(70, 8)),                             # out dtype
    dict(a=torch.zeros(70, 256, dtype=BF16, device="meta")),  # device
], ids=lambda c: "+".join(c))
def test_gemm_argument_errors(change):
    w4, w_scale = random_pack(8, 256, seed=3)
    args = dict(a=torch.zeros(70, 256, dtype=BF16), w4=w4, w_scale=w_scale)
    with pytest.raises(ValueError):
        ops.gemm_mxfp4(**{**args, **change})


def test_mode_errors_without_a_gpu():
    cfg = LlamaConfig.tiny(hidden_size=128, intermediate_size=256,
                           vocab_size=512)
    with pytest.raises(ValueError, match="prefill_gemm.*weight_dtype"):
        LlamaDecodeEngine(cfg, batch_size=2, device="cpu",
                          prefill_gemm="mxfp4")               # bf16 weights
    with pytest.raises(ValueError, match="unknown prefill_gemm"):
        LlamaDecodeEngine(cfg, batch_size=2, device="cpu",
                          prefill_gemm="hipblaslt")
    engine = LlamaDecodeEngine(cfg, batch_size=2, device="cpu")
    with pytest.raises(ValueError, match="prefill_gemm"):
        engine.release_master_weights()
    assert engine.weights.lm_head is not None
    server = LlamaServer(name="gen", config="tiny", batch_size=2,
                         device="cpu", release_masters=True)
    with pytest.raises(ValueError, match="release_masters.*prefill_gemm"):
        server.load()
    assert server.engines == []
