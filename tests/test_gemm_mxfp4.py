# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""MXFP4 weight mode without a GPU: quantizer, packs, CPU GEMM, errors."""

import pytest
import torch

from mlrun_amd import ops
from mlrun_amd.models.llama import LlamaConfig, LlamaDecodeEngine, LlamaServer

from decode_refs import EPS32, R1, check, f64

MAGS = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
TABLE = torch.tensor(MAGS + tuple(-v for v in MAGS), dtype=torch.float64)
BF16 = torch.bfloat16


def logical_scales(w_scale):
    out = torch.empty_like(w_scale)
    out[:, ops._mxfp4_scale_order(w_scale.shape[1], "cpu")] = w_scale
    return out


def dequant64(w4, w_scale):
    codes = torch.stack([w4 & 0xF, w4 >> 4], dim=-1).flatten(1).long()
    e = logical_scales(w_scale).to(torch.float64) - 127
    return TABLE[codes] * (2.0 ** e).repeat_interleave(32, dim=1)


def random_pack(n, k, seed):
    g = torch.Generator().manual_seed(seed)
    w4 = torch.randint(0, 256, (n, k // 2), generator=g)
    scale = torch.randint(127 - 20, 127 + 11, (n, k // 32), generator=g)
    return w4.to(torch.uint8), scale.to(torch.uint8)


def test_quantize_matches_brute_force():
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(6, 256, generator=g) * 3).to(BF16)
    w[0, :32] = w[1, 32:64] = 0                     # all-zero block
    w[1, 40] = 2.0 ** -130                          # exponent clamp
    w[2, 64:96] = (torch.rand(32, generator=g) * 4).to(BF16)
    w[2, 70] = 7.5                                  # e = 0: saturates at 6
    w[3, 0:4] = torch.tensor([2.5, -2.5, 3.5, 5.0])  # ties, amax in [4, 8)
    w4, w_scale = ops.quantize_mxfp4_weight(w)
    x = f64(w).view(6, 8, 32)
    amax = x.abs().amax(-1)
    e = torch.floor(torch.log2(amax.clamp_min(2.0 ** -200))) - 2
    e = torch.where(amax == 0, torch.zeros_like(e), e.clamp(-120, 120))
    cand = torch.tensor([0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15])
    dist = (x[..., None] / 2.0 ** e[..., None, None] - TABLE[cand]).abs()
    dist = dist + (cand % 2) * 1e-9                 # exact ties: even code
    got = torch.stack([w4 & 0xF, w4 >> 4], dim=-1).view(6, 256).long()
    assert torch.equal(got, cand[dist.argmin(-1)].view(6, 256))
    assert torch.equal(logical_scales(w_scale).long(), (e + 127).long())


def test_round_trip_is_identity_and_bad_weights_raise():
    w4, w_scale = random_pack(5, 640, seed=1)
    w = ops.dequantize_mxfp4_weight(w4, w_scale)
    assert w.dtype == BF16 and torch.equal(f64(w), dequant64(w4, w_scale))
    again = ops.dequantize_mxfp4_weight(*ops.quantize_mxfp4_weight(w))
    assert torch.equal(again, w)
    for bad in (torch.zeros(4, 192, dtype=BF16), torch.zeros(4, 128),
                torch.zeros(128, dtype=BF16)):      # K % 128, dtype, rank
        with pytest.raises(ValueError):
            ops.quantize_mxfp4_weight(bad)


@pytest.mark.parametrize("m,n,k", [(3, 40, 640), (64, 7, 128)])
def test_cpu_gemm_against_float64(m, n, k):
    w4, w_scale = random_pack(n, k, seed=k + m)
    a = torch.randn(m, k, generator=torch.Generator().manual_seed(2)).to(BF16)
    w = dequant64(w4, w_scale)
    ref = f64(a) @ w.t()
    bound = R1 * ref.abs() + (k + 3) * EPS32 * (f64(a).abs() @ w.abs().t()) \
        * (1 + R1)
    out = torch.empty(m, n, dtype=BF16)
    assert ops.skinny_gemm_mxfp4(a, w4, w_scale, out=out) is out
    check(out, ref, bound, f"cpu mxfp4 gemm m{m} n{n} k{k}")


@pytest.mark.parametrize("change", [
    dict(a=torch.zeros(2, 256)),                              # dtype
    dict(a=torch.zeros(256, dtype=BF16)),                     # rank
    dict(a=torch.zeros(256, 2, dtype=BF16).t()),              # contiguity
    dict(a=torch.zeros(65, 256, dtype=BF16)),                 # M > 64
    dict(a=torch.zeros(2, 128, dtype=BF16)),                  # K mismatch
    dict(a=torch.zeros(2, 192, dtype=BF16),
         w4=torch.zeros(8, 96, dtype=torch.uint8),
         w_scale=torch.zeros(8, 6, dtype=torch.uint8)),       # K % 128
    dict(w_scale=torch.zeros(7, 8, dtype=torch.uint8)),       # N mismatch
    dict(w4=torch.zeros(8, 128, dtype=torch.int8)),           # dtype
    dict(out=torch.zeros(2, 9, dtype=BF16)),                  # out shape
    dict(ksplit=2, c_f32=torch.zeros(31)),                    # scratch
    dict(ksplit=0), dict(ksplit=129),
    dict(a=torch.zeros(2, 256, dtype=BF16, device="meta")),   # device
], ids=lambda c: "+".join(c))
def test_gemm_argument_errors(change):
    w4, w_scale = random_pack(8, 256, seed=3)
    args = dict(a=torch.zeros(2, 256, dtype=BF16), w4=w4, w_scale=w_scale)
    with pytest.raises(ValueError):
        ops.skinny_gemm_mxfp4(**{**args, **change})


def test_mode_without_a_gpu():
    with pytest.raises(ValueError, match='weight_dtype="mxfp4w"'):
        LlamaServer(name="gen", config="tiny", batch_size=2, device="cpu",
                    weight_dtype="mxfp4w", speculative=2).load()
    cfg = LlamaConfig.tiny(hidden_size=128, intermediate_size=256,
                           vocab_size=512)
    prompt = torch.randint(0, 500, (2, 5),
                           generator=torch.Generator().manual_seed(4))
    ref, mx4 = [LlamaDecodeEngine(cfg, batch_size=2, device="cpu", seed=7,
                                  weight_dtype=mode)
                for mode in ("bf16", "mxfp4w")]   # both run the masters
    mx4.rebuild_weight_packs()
    assert mx4._mx4_packs == {}
    assert torch.equal(mx4.generate(prompt, max_new_tokens=3),
                       ref.generate(prompt, max_new_tokens=3))
