# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""The bf16 tile GEMM (gemm_bf16_tile_kernel) against float64, its fixed
summation order, and the bf16 engine that prefills on it."""

import functools

import pytest
import torch

from mlrun_amd import ops
from mlrun_amd.models.llama import LlamaConfig, LlamaDecodeEngine

from decode_refs import EPS32, R1, check, f64

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs MI355X")]
MASTERS = ("wqkv", "wo", "wgu", "wdown")
TINY = dict(num_layers=2, num_heads=4, num_kv_heads=2, hidden_size=512,
            intermediate_size=1024, vocab_size=2048)


@functools.lru_cache(maxsize=None)
def case(m, n, k):
    """Seeded N(0,1) bf16 operands, the float64 product of their values,
    and the bound: exact products, K fp32 additions, one bf16 rounding."""
    g = torch.Generator().manual_seed(10 * k + m + n)
    a = torch.randn(m, k, generator=g).to(torch.bfloat16)
    w = torch.randn(n, k, generator=g).to(torch.bfloat16)
    ref = f64(a) @ f64(w).t()
    magnitude = f64(a).abs() @ f64(w).abs().t()
    return a, w, ref, R1 * ref.abs() + (k + 2) * EPS32 * magnitude


def gemm(bn, a, w, out=None):
    """bn 0: the public op, which picks 64-wide tiles at shapes this
    small.  bn 64 / 128: that instance of the kernel, through the binding."""
    if bn == 0:
        return ops.gemm_bf16(a, w, out=out)
    if out is None:
        out = torch.empty(a.shape[0], w.shape[0], dtype=torch.bfloat16,
                          device=a.device)
    ops._require_hip().gemm_bf16_tile(out, a, w, bn)
    return out


# M: one or two M tiles, full and ragged; N: one clamped tile, an exact
# one, several with a ragged last; K: the 32-k tail alone, one stage, a
# stage plus the tail, a long loop ending in a tail.
@pytest.mark.parametrize("bn", [0, 128])
@pytest.mark.parametrize("k", [32, 64, 96, 1120])
@pytest.mark.parametrize("n", [80, 128, 272])
@pytest.mark.parametrize("m", [65, 128, 129, 200])
def test_kernel_against_float64(m, n, k, bn):
    a, w, ref, bound = case(m, n, k)
    check(gemm(bn, a.cuda(), w.cuda()), ref, bound,
          f"bf16 tile gemm m{m} n{n} k{k} bn{bn}", kernel="gemm_bf16_tile")


@pytest.mark.parametrize("bn", [64, 128])
def test_memory_past_the_operands_is_never_read(bn):
    """Each operand ends its buffer and bf16 NaN follows; out sits between
    sentinel rows, which stay."""
    m, n, k = 129, 80, 96
    a, w, ref, bound = case(m, n, k)

    def guarded(t):
        buf = torch.full((2 * t.numel(),), float("nan"), dtype=t.dtype,
                         device="cuda")
        buf[:t.numel()] = t.flatten().cuda()
        return buf[:t.numel()].view(t.shape)

    # 8 rows of n keep out 16-byte aligned
    frame = torch.full((m + 16, n), 77.0, dtype=torch.bfloat16, device="cuda")
    out = frame[8:8 + m]
    gemm(bn, guarded(a), guarded(w), out)
    assert (frame[:8] == 77.0).all() and (frame[8 + m:] == 77.0).all()
    check(out, ref, bound, f"bf16 tile gemm guarded bn{bn}")


def test_bits_depend_on_the_row_the_column_and_k_alone():
    m, n, k = 200, 272, 1120
    a, w = (t.cuda() for t in case(m, n, k)[:2])
    full = gemm(0, a, w)
    assert torch.equal(full[:65], gemm(0, a[:65], w))
    perm = torch.randperm(m, generator=torch.Generator().manual_seed(2)).cuda()
    assert torch.equal(full[perm], gemm(0, a[perm].contiguous(), w))
    assert torch.equal(full[:, :80], gemm(0, a, w[:80]))
    for bn in (64, 128):
        assert torch.equal(full, gemm(bn, a, w)), f"bn {bn}"


def two_steps(engine, prompt):
    first = f64(engine.prefill(prompt))
    engine.buf_tokens.copy_(first.argmax(dim=-1))
    engine.decode_step()
    return first, f64(engine.buf_logits)


def test_engine_prefill_on_tile_kernel_matches_library_on_same_weights():
    """X prefills 96 rows with the tile kernel, R with the library GEMM on
    the same weights: one function, two summation orders.  Tolerance
    2 * R1 * |ref| + 2 * spread, spread that of a bf16 engine on the same
    weights against itself under split-K plans 1 and 2."""
    cfg, B = LlamaConfig.tiny(**TINY), 8
    prompt = torch.randint(0, 2000, (B, 12),
                           generator=torch.Generator().manual_seed(8))

    def engine(prefill_gemm):
        return LlamaDecodeEngine(cfg, batch_size=B, device="cuda:0",
                                 use_graph=False, seed=41,
                                 prefill_gemm=prefill_gemm)

    y = engine("library")
    shapes = [tuple(y.weights.lm_head.shape)] + [
        tuple(y.weights.layers[0][name].shape) for name in MASTERS]
    plans = []
    for ksplit in (1, 2):
        y._ksplits = {shape: (ksplit, 1) for shape in shapes}
        plans.append(two_steps(y, prompt)[1])
        y.reset()
    spread = (plans[0] - plans[1]).abs().max().item()
    print(f"bf16 spread {spread:.4g}")
    refs = two_steps(engine("library"), prompt)
    gots = two_steps(engine("bf16"), prompt)
    for what, got, ref in zip(("prefill", "decode step"), gots, refs):
        check(got, ref, 2 * R1 * ref.abs() + 2 * spread,
              f"bf16 prefill engine, {what} logits vs library prefill")
