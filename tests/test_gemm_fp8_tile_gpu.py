# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""The fp8 tile GEMM (gemm_fp8_tile_kernel) against float64, and the fp8w
engine that prefills on the packs and releases the bf16 masters."""

import functools

import pytest
import torch

from mlrun_amd import ops
from mlrun_amd.models.llama import LlamaConfig, LlamaDecodeEngine

from decode_refs import check, f64, gemm_fp8_case, gemm_fp8_reference

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs MI355X")]
MASTERS = ("wqkv", "wo", "wgu", "wdown")
TINY = dict(num_layers=2, num_heads=4, num_kv_heads=2, hidden_size=512,
            intermediate_size=1024, vocab_size=2048)


@functools.lru_cache(maxsize=None)
def expected(m, k, n):
    return gemm_fp8_reference(*gemm_fp8_case(m, k, n), ksplit=1)


def gemm(bn, a8, a_scale, w8, w_scale, out=None):
    """bn 0: the public op, which picks 64-wide tiles at shapes this
    small.  bn 128: the kernel's wide instance, through the binding."""
    if bn == 0:
        return ops.gemm_fp8(a8, a_scale, w8, w_scale, out=out)
    if out is None:
        out = torch.empty(a8.shape[0], w8.shape[0], dtype=torch.bfloat16,
                          device=a8.device)
    ops._require_hip().gemm_fp8_tile(out, a8, a_scale, w8, w_scale, bn)
    return out


# M: one or two M tiles, full and ragged; N: one clamped tile, an exact
# one, several with a ragged last; K: the 64-byte tail step alone, one
# full step, a full step plus the tail, a long loop ending in a tail.
@pytest.mark.parametrize("bn", [0, 128])
@pytest.mark.parametrize("k", [64, 128, 192, 1088])
@pytest.mark.parametrize("n", [80, 128, 272])
@pytest.mark.parametrize("m", [65, 128, 129, 200])
def test_kernel_against_float64(m, n, k, bn):
    got = gemm(bn, *(t.cuda() for t in gemm_fp8_case(m, k, n)))
    check(got, *expected(m, k, n), f"fp8 tile gemm m{m} n{n} k{k} bn{bn}",
          kernel="gemm_fp8_tile")


@pytest.mark.parametrize("bn", [0, 128])
def test_memory_past_the_operands_is_never_read(bn):
    """Each operand ends its buffer and NaN follows (e4m3 code 0x7F, f32
    NaN scales); out sits between sentinel rows, which stay."""
    m, n, k = 129, 80, 192
    case = gemm_fp8_case(m, k, n)

    def guarded(t, fill):
        buf = torch.full((2 * t.numel(),), fill, dtype=t.dtype, device="cuda")
        buf[:t.numel()] = t.flatten().cuda()
        return buf[:t.numel()].view(t.shape)

    a8, w8 = guarded(case[0], 0x7F), guarded(case[2], 0x7F)
    a_scale = guarded(case[1], float("nan"))
    w_scale = guarded(case[3], float("nan"))
    # 8 rows of n keep out 16-byte aligned
    frame = torch.full((m + 16, n), 77.0, dtype=torch.bfloat16, device="cuda")
    out = frame[8:8 + m]
    gemm(bn, a8, a_scale, w8, w_scale, out)
    assert (frame[:8] == 77.0).all() and (frame[8 + m:] == 77.0).all()
    check(out, *expected(m, k, n), f"fp8 tile gemm guarded bn{bn}")


def fp8_engine(cfg, B, prefill_gemm):
    return LlamaDecodeEngine(cfg, batch_size=B, device="cuda:0",
                             use_graph=False, seed=41, weight_dtype="fp8w",
                             prefill_gemm=prefill_gemm)


def test_engine_prefill_and_decode_are_one_model_and_masters_go():
    """X prefills 2 x 96 rows with the tile kernel on the packs, Y with
    the library GEMM on the bf16 masters of the same weights.  The 96
    tokens fed one at a time through X's decode step are the quantized
    model's own answer: X's prefill must be closer to it than Y's.
    Measured on MI355X: d_fp8 0.1055, d_lib 0.2041 (docs/kernels.md).
    Then X releases its masters and computes what it computed before."""
    cfg, B, S = LlamaConfig.tiny(**TINY), 2, 96
    prompt = torch.randint(0, 2000, (B, S),
                           generator=torch.Generator().manual_seed(8))
    x, y = fp8_engine(cfg, B, "fp8"), fp8_engine(cfg, B, "library")
    y._fp8_packs = x._fp8_packs
    pre_x, pre_y = f64(x.prefill(prompt)), f64(y.prefill(prompt))
    x.reset()
    for t in range(S):
        x.buf_tokens.copy_(prompt[:, t])
        x.decode_step()
    fed = f64(x.buf_logits)
    d_fp8 = (pre_x - fed).abs().max().item()
    d_lib = (pre_y - fed).abs().max().item()
    print(f"d_fp8 {d_fp8:.4g}  d_lib {d_lib:.4g}")
    assert d_fp8 < d_lib

    x.reset()
    tokens = x.generate(prompt, max_new_tokens=4)
    freed = sum(t.numel() * t.element_size() for t in [x.weights.lm_head] + [
        layer[name] for layer in x.weights.layers for name in MASTERS])
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    x.release_master_weights()
    assert held - torch.cuda.memory_allocated() >= freed > 0
    assert x.weights.lm_head is None and all(
        layer[name] is None for layer in x.weights.layers for name in MASTERS)
    x.reset()
    assert torch.equal(x.generate(prompt, max_new_tokens=4), tokens)
    x.reset()
    assert torch.equal(f64(x.prefill(prompt)), pre_x)
    for call in (x.rebuild_weight_packs, x.weights.state_dict):
        with pytest.raises(ValueError, match="released"):
            call()
