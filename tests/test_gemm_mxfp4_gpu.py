# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""The MXFP4 decode GEMM and the mxfp4w engine mode against float64."""

import functools

import pytest
import torch

from mlrun_amd import ops
from mlrun_amd.models.llama import (LlamaConfig, LlamaDecodeEngine,
                                    LlamaWeights)

from decode_refs import EPS32, R1, check, f64
from test_gemm_mxfp4 import TABLE

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs MI355X")]
TINY = dict(num_layers=2, num_heads=4, num_kv_heads=2, hidden_size=512,
            intermediate_size=1024, vocab_size=2048)


@functools.lru_cache(None)
def gemm_case(m, n, k):
    """All 16 codes; scale bytes of neighbouring blocks and rows differ, so
    a scale or block from the wrong place is off by 2x or more."""
    g = torch.Generator().manual_seed(10 * k + m)
    codes = torch.randint(0, 16, (n, k), generator=g)
    w4 = (codes[:, 0::2] | (codes[:, 1::2] << 4)).to(torch.uint8)
    byte = 120 + (3 * torch.arange(n)[:, None] +
                  5 * torch.arange(k // 32)[None, :]) % 11
    w = TABLE[codes] * (2.0 ** (byte - 127.0)).repeat_interleave(32, dim=1)
    w_scale = byte[:, ops._mxfp4_scale_order(k // 32, "cpu")].to(torch.uint8)
    step = 1.25 ** ((3 * torch.arange(m)) % 17).float()
    a = (torch.randn(m, k, generator=g) * step[:, None]).to(torch.bfloat16)
    return a, w4, w_scale.contiguous(), w


def check_gemm(got, a, w, ksplit, what):
    """Exact products, K fp32 additions, ksplit slabs, one bf16 rounding."""
    ref = f64(a) @ w.t()
    acc = (a.shape[1] + ksplit + 2) * EPS32 * (f64(a).abs() @ w.abs().t())
    check(got, ref, R1 * ref.abs() + acc * (1 + R1), what,
          kernel="skinny_gemm_mxfp4")


# K 4224 (33 super-steps), M <= 16, ksplit 1: waves own 1152 k, each runs
# the four-step body behind 0..3 single steps and before single steps, the
# last in the ungrouped scale tail; ksplit 2: waves of 640 k, body first.
@pytest.mark.parametrize("m,n,k,ksplit",
                         [(m, 80, k, s) for m in (1, 16, 17, 32, 33, 64)
                          for k in (128, 384, 1152) for s in (1, 2, 5)] +
                         [(32, 64, 512, 1)] +
                         [(m, 80, 4224, s) for m in (1, 16) for s in (1, 2)])
def test_kernel_against_float64(m, n, k, ksplit):
    a, w4, w_scale, w = gemm_case(m, n, k)
    got = ops.skinny_gemm_mxfp4(a.cuda(), w4.cuda(), w_scale.cuda(),
                                ksplit=ksplit)
    check_gemm(got, a, w, ksplit, f"mxfp4 gemm m{m} n{n} k{k} ks{ksplit}")


@pytest.mark.parametrize("ksplit", [1, 2])
def test_padding_rows_are_never_read(ksplit):
    """Each operand ends its buffer and NaN (bf16 NaN, scale byte 0xFF)
    follows; out beyond [M, N] keeps its sentinel."""
    m, n, k = 17, 80, 384
    a, w4, w_scale, w = gemm_case(m, n, k)

    def guarded(t, fill):
        buf = torch.full((2 * t.numel(),), fill, dtype=t.dtype, device="cuda")
        buf[:t.numel()] = t.flatten().cuda()
        return buf[:t.numel()].view(t.shape)

    out = guarded(torch.zeros(m, n, dtype=torch.bfloat16), 77.0)
    ops.skinny_gemm_mxfp4(
        guarded(a, float("nan")), guarded(w4, 0xFF), guarded(w_scale, 0xFF),
        out=out, c_f32=torch.empty(ksplit * m * n, device="cuda"),
        ksplit=ksplit)
    assert torch.isfinite(out).all()
    assert (torch.as_strided(out, (m * n,), (1,), m * n) == 77.0).all()
    check_gemm(out, a, w, ksplit, f"mxfp4 gemm guarded ks{ksplit}")


def step_logits(engine, prompt):
    engine.buf_tokens.copy_(engine.prefill(prompt).argmax(dim=-1))
    engine.decode_step()
    return f64(engine.buf_logits)


def test_engine_matches_bf16_engine_on_dequantized_weights():
    """X (mxfp4w) and Y (bf16) hold the dequantized packs: one function,
    two summation orders.  Logits agree within 2 * R1 * |y| + a, a twice
    the spread of Y against itself under two split-K plans (measured on
    MI355X: spread 0.0117, a = 0.0234, |logit| <= 1.7).  Rows whose
    top-two gap exceeds the tolerance give the same token; at most 2 of 8
    rows may fall under the gap rule.  Weights (CPU generator, seed 41)
    and prompt (seed 8) leave all 8 rows of the CPU bf16 reference clear
    at a = 0.0312."""
    cfg, B = LlamaConfig.tiny(**TINY), 8
    prompt = torch.randint(0, 2000, (B, 8),
                           generator=torch.Generator().manual_seed(8))
    x = LlamaDecodeEngine(cfg, batch_size=B, device="cuda:0",
                          use_graph=False, seed=1, weight_dtype="mxfp4w")
    x.weights.load_state_dict(LlamaWeights(cfg, "cpu", seed=41).state_dict())
    x.rebuild_weight_packs()    # re-quantize from the loaded weights
    masters = [x.weights.lm_head] + [layer[key] for layer in x.weights.layers
                                     for key in ("wqkv", "wo", "wgu", "wdown")]
    for master in masters:      # the round trip keeps X's packs valid
        master.copy_(ops.dequantize_mxfp4_weight(*x._mx4_packs[id(master)]))
    y = LlamaDecodeEngine(cfg, batch_size=B, device="cuda:0",
                          use_graph=False, seed=1)
    y.weights.load_state_dict(x.weights.state_dict())
    plans = []
    for ksplit in (1, 2):
        y._ksplits = {tuple(master.shape): (ksplit, 1) for master in masters}
        plans.append(step_logits(y, prompt))
    ref, spread = plans[0], (plans[0] - plans[1]).abs().max().item()
    tol = 2 * R1 * ref.abs() + 2 * spread
    print(f"bf16 spread {spread:.4g}, max |logit| {ref.abs().max():.3g}")
    got = step_logits(x, prompt)
    check(got, ref, tol, "mxfp4w engine logits vs bf16 on the same weights")
    top2 = ref.topk(2, dim=-1)
    clear = (top2.values[:, 0] - top2.values[:, 1]) > \
        tol.gather(1, top2.indices).sum(dim=-1)
    assert int(clear.sum()) >= B - B // 4
    assert torch.equal(got.argmax(-1)[clear], ref.argmax(-1)[clear])


def test_graph_replay_matches_eager():
    prompt = torch.randint(0, 2000, (4, 8),
                           generator=torch.Generator().manual_seed(5))
    tokens = [LlamaDecodeEngine(LlamaConfig.tiny(**TINY), batch_size=4,
                                device="cuda:0", use_graph=graph, seed=41,
                                weight_dtype="mxfp4w")
              .generate(prompt, max_new_tokens=4) for graph in (False, True)]
    assert torch.equal(tokens[0], tokens[1])
