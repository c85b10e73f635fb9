# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""The any-M fp8 GEMM and the fp8 prefill mode without a GPU."""

import pytest
import torch

from mlrun_amd import ops
from mlrun_amd.models.llama import LlamaConfig, LlamaDecodeEngine, LlamaServer

from decode_refs import check, gemm_fp8_case, gemm_fp8_reference

U8, F32, BF16 = torch.uint8, torch.float32, torch.bfloat16


def test_cpu_gemm_against_float64():
    m, k, n = 70, 192, 80
    case = gemm_fp8_case(m, k, n)
    out = torch.empty(m, n, dtype=BF16)
    assert ops.gemm_fp8(*case, out=out) is out
    check(out, *gemm_fp8_reference(*case, ksplit=1, mfma=False),
          f"cpu fp8 gemm m{m} n{n} k{k}")


@pytest.mark.parametrize("change", [
    dict(a8=torch.zeros(70, 128, dtype=torch.int8)),             # dtype
    dict(w_scale=torch.zeros(8, dtype=torch.float64)),           # dtype
    dict(a8=torch.zeros(128, dtype=U8)),                         # rank
    dict(a_scale=torch.zeros(70, 1)),                            # rank
    dict(a8=torch.zeros(128, 70, dtype=U8).t()),                 # contiguity
    dict(a8=torch.zeros(0, 128, dtype=U8),
         a_scale=torch.zeros(0)),                                # M < 1
    dict(a8=torch.zeros(70, 64, dtype=U8)),                      # K mismatch
    dict(a8=torch.zeros(70, 96, dtype=U8),
         w8=torch.zeros(8, 96, dtype=U8)),                       # K % 64
    dict(a_scale=torch.zeros(69)),                               # M scales
    dict(w_scale=torch.zeros(9)),                                # N scales
    dict(out=torch.zeros(70, 9, dtype=BF16)),                    # out shape
    dict(out=torch.zeros(70, 8)),                                # out dtype
    dict(a8=torch.zeros(70, 128, dtype=U8, device="meta")),      # device
], ids=lambda c: "+".join(c))
def test_gemm_argument_errors(change):
    args = dict(a8=torch.zeros(70, 128, dtype=U8), a_scale=torch.ones(70),
                w8=torch.zeros(8, 128, dtype=U8), w_scale=torch.ones(8))
    ops.gemm_fp8(**args)
    with pytest.raises(ValueError):
        ops.gemm_fp8(**{**args, **change})


def test_mode_errors_without_a_gpu():
    cfg = LlamaConfig.tiny(hidden_size=128, intermediate_size=256,
                           vocab_size=512)
    for weight_dtype in ("bf16", "mxfp4w", "fp8w"):     # fp8w: not on a cpu
        with pytest.raises(ValueError, match="prefill_gemm.*weight_dtype"):
            LlamaDecodeEngine(cfg, batch_size=2, device="cpu",
                              weight_dtype=weight_dtype, prefill_gemm="fp8")
    engine = LlamaDecodeEngine(cfg, batch_size=2, device="cpu",
                               weight_dtype="fp8w")
    with pytest.raises(ValueError, match="prefill_gemm"):
        engine.release_master_weights()
    assert engine.weights.lm_head is not None
    for prefill_gemm in ("library", "fp8"):
        server = LlamaServer(name="gen", config="tiny", batch_size=2,
                             device="cpu", release_masters=True,
                             prefill_gemm=prefill_gemm)
        with pytest.raises(ValueError,
                           match="release_masters.*prefill_gemm"
                           if prefill_gemm == "library"
                           else "prefill_gemm.*weight_dtype"):
            server.load()
        assert server.engines == []
