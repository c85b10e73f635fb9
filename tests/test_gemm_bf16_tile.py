# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""The any-M bf16 GEMM and the bf16 prefill mode without a GPU."""

import pytest
import torch

from mlrun_amd import ops
from mlrun_amd.models.llama import LlamaConfig, LlamaDecodeEngine

BF16 = torch.bfloat16


@pytest.mark.parametrize("change", [
    dict(a=torch.zeros(70, 64)),                                # dtype
    dict(w=torch.zeros(8, 64, dtype=torch.float16)),            # dtype
    dict(a=torch.zeros(64, dtype=BF16)),                        # rank
    dict(w=torch.zeros(1, 8, 64, dtype=BF16)),                  # rank
    dict(a=torch.zeros(64, 70, dtype=BF16).t()),                # contiguity
    dict(a=torch.zeros(0, 64, dtype=BF16)),                     # M < 1
    dict(a=torch.zeros(70, 32, dtype=BF16)),                    # K mismatch
    dict(a=torch.zeros(70, 48, dtype=BF16),
         w=torch.zeros(8, 48, dtype=BF16)),                     # K % 32
    dict(out=torch.zeros(70, 9, dtype=BF16)),                   # out shape
    dict(out=torch.zeros(70, 8)),                               # out dtype
    dict(out=torch.zeros(8, 70, dtype=BF16).t()),               # out layout
    dict(a=torch.zeros(70, 64, dtype=BF16, device="meta")),     # device
], ids=lambda c: "+".join(c))
def test_gemm_argument_errors(change):
    args = dict(a=torch.zeros(70, 64, dtype=BF16),
                w=torch.zeros(8, 64, dtype=BF16))
    out = torch.empty(70, 8, dtype=BF16)
    assert ops.gemm_bf16(**args, out=out) is out
    with pytest.raises(ValueError):
        ops.gemm_bf16(**{**args, **change})


def test_mode_errors_and_cpu_engine_equals_the_default():
    cfg = LlamaConfig.tiny(hidden_size=128, intermediate_size=256,
                           vocab_size=512)
    for weight_dtype in ("fp8w", "mxfp4w"):
        with pytest.raises(ValueError, match="prefill_gemm.*weight_dtype"):
            LlamaDecodeEngine(cfg, batch_size=2, device="cpu",
                              weight_dtype=weight_dtype, prefill_gemm="bf16")
    engines = [LlamaDecodeEngine(cfg, batch_size=2, device="cpu", seed=5,
                                 prefill_gemm=mode)
               for mode in ("bf16", "library")]
    with pytest.raises(ValueError, match="prefill_gemm"):
        engines[0].release_master_weights()
    assert engines[0].weights.lm_head is not None
    prompt = torch.randint(0, 500, (2, 9),
                           generator=torch.Generator().manual_seed(3))
    assert torch.equal(*(e.prefill(prompt) for e in engines))
