# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""The mxfp4 tile GEMM against float64, and the engine / server that
prefill on the packs and release the bf16 masters."""

import pytest
import torch

from mlrun_amd import ops
from mlrun_amd.models.llama import (LlamaConfig, LlamaDecodeEngine,
                                    LlamaServer, LlamaWeights)

from decode_refs import R1, check, f64
from test_gemm_mxfp4_gpu import TINY, check_gemm, gemm_case

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs MI355X")]
MASTERS = ("wqkv", "wo", "wgu", "wdown")


def gemm(bn, a, w4, w_scale, out=None):
    """bn 0: the public op.  bn 128: the tile kernel's wide instance,
    which the launcher does not choose at shapes this small."""
    if bn == 0 or a.shape[0] <= 64:
        return ops.gemm_mxfp4(a, w4, w_scale, out=out)
    if out is None:
        out = torch.empty(a.shape[0], w4.shape[0], dtype=a.dtype,
                          device=a.device)
    ops._require_hip().gemm_mxfp4_tile(out, a, w4, w_scale, bn)
    return out


# M: one or two M tiles, full and ragged; N: one clamped tile, an exact one,
# three with a ragged last; K: one step, tail-order scales only, a full scale
# group plus a tail, two groups plus a tail.  bn 0 picks 64-wide tiles at
# these sizes, 128 forces the wide kernel; (8, 80, 384) is the skinny kernel.
@pytest.mark.parametrize("bn", [0, 128])
@pytest.mark.parametrize("m,n,k",
                         [(m, n, k) for m in (65, 128, 129, 200)
                          for n in (80, 128, 272)
                          for k in (128, 384, 640, 1152)] + [(8, 80, 384)])
def test_kernel_against_float64(m, n, k, bn):
    a, w4, w_scale, w = gemm_case(m, n, k)
    got = gemm(bn, a.cuda(), w4.cuda(), w_scale.cuda())
    check_gemm(got, a, w, 0, f"mxfp4 tile gemm m{m} n{n} k{k} bn{bn}")


@pytest.mark.parametrize("bn", [0, 128])
def test_padding_rows_are_never_read(bn):
    """Each operand ends its buffer and NaN (bf16 NaN, scale byte 0xFF)
    follows; out beyond [M, N] keeps its sentinel."""
    m, n, k = 129, 80, 384
    a, w4, w_scale, w = gemm_case(m, n, k)

    def guarded(t, fill):
        buf = torch.full((2 * t.numel(),), fill, dtype=t.dtype, device="cuda")
        buf[:t.numel()] = t.flatten().cuda()
        return buf[:t.numel()].view(t.shape)

    out = guarded(torch.zeros(m, n, dtype=torch.bfloat16), 77.0)
    gemm(bn, guarded(a, float("nan")), guarded(w4, 0xFF),
         guarded(w_scale, 0xFF), out)
    assert torch.isfinite(out).all()
    assert (torch.as_strided(out, (m * n,), (1,), m * n) == 77.0).all()
    check_gemm(out, a, w, 0, f"mxfp4 tile gemm guarded bn{bn}")


def mx4_engine(cfg, B, prefill_gemm):
    """An mxfp4w engine on the seed-41 weights, its masters overwritten
    with the dequantized packs (the round trip keeps the packs valid)."""
    e = LlamaDecodeEngine(cfg, batch_size=B, device="cuda:0", use_graph=False,
                          seed=1, weight_dtype="mxfp4w",
                          prefill_gemm=prefill_gemm)
    e.weights.load_state_dict(LlamaWeights(cfg, "cpu", seed=41).state_dict())
    e.rebuild_weight_packs()
    e.weights.lm_head.copy_(
        ops.dequantize_mxfp4_weight(*e._mx4_packs["lm_head"]))
    for li, layer in enumerate(e.weights.layers):
        for name in MASTERS:
            layer[name].copy_(
                ops.dequantize_mxfp4_weight(*e._mx4_packs[(li, name)]))
    return e


def two_steps(engine, prompt):
    first = f64(engine.prefill(prompt))
    engine.buf_tokens.copy_(first.argmax(dim=-1))
    engine.decode_step()
    return first, f64(engine.buf_logits)


def test_engine_prefill_on_packs_matches_library_on_same_weights():
    """X prefills 96 rows with the tile kernel on the packs, R with the
    library GEMM on the dequantized packs: one function, two summation
    orders.  Tolerance 2 * R1 * |ref| + 2 * spread, spread that of a
    bf16 engine on the same weights against itself under split-K plans
    1 and 2."""
    cfg, B = LlamaConfig.tiny(**TINY), 8
    prompt = torch.randint(0, 2000, (B, 12),
                           generator=torch.Generator().manual_seed(8))
    r = mx4_engine(cfg, B, "library")
    y = LlamaDecodeEngine(cfg, batch_size=B, device="cuda:0",
                          use_graph=False, seed=1)
    y.weights.load_state_dict(r.weights.state_dict())
    shapes = [tuple(r.weights.lm_head.shape)] + [
        tuple(r.weights.layers[0][name].shape) for name in MASTERS]
    plans = []
    for ksplit in (1, 2):
        y._ksplits = {shape: (ksplit, 1) for shape in shapes}
        plans.append(two_steps(y, prompt)[1])
    spread = (plans[0] - plans[1]).abs().max().item()
    refs = two_steps(r, prompt)
    gots = two_steps(mx4_engine(cfg, B, "mxfp4"), prompt)
    print(f"bf16 spread {spread:.4g}")
    for what, got, ref in zip(("prefill", "decode step"), gots, refs):
        check(got, ref, 2 * R1 * ref.abs() + 2 * spread,
              f"mxfp4 prefill engine, {what} logits vs library prefill")


def test_release_frees_the_masters_and_changes_nothing():
    cfg, B = LlamaConfig.tiny(**TINY), 8
    prompt = torch.randint(0, 2000, (B, 12),
                           generator=torch.Generator().manual_seed(8))
    x = LlamaDecodeEngine(cfg, batch_size=B, device="cuda:0", use_graph=False,
                          seed=41, weight_dtype="mxfp4w",
                          prefill_gemm="mxfp4")
    before = x.generate(prompt, max_new_tokens=4)
    freed = sum(t.numel() * t.element_size() for t in [x.weights.lm_head] + [
        layer[name] for layer in x.weights.layers for name in MASTERS])
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    x.release_master_weights()
    assert held - torch.cuda.memory_allocated() >= freed
    x.reset()
    assert torch.equal(x.generate(prompt, max_new_tokens=4), before)
    for call in (x.rebuild_weight_packs, x.weights.state_dict):
        with pytest.raises(ValueError, match="released"):
            call()


def test_server_serves_without_masters():
    server = LlamaServer(name="gen", config=LlamaConfig.tiny(**TINY),
                         batch_size=4, device="cuda:0", max_new_tokens=4,
                         weight_dtype="mxfp4w", prefill_gemm="mxfp4",
                         release_masters=True, scheduling="continuous",
                         prefill="packed")
    server.load()

    class Event:
        id, path = "ev", ""
        body = {"inputs": [[1, 2, 3], [4, 5, 6, 7, 8], list(range(20, 90))],
                "max_tokens": 4}

    try:
        assert server.engine.weights.lm_head is None
        outputs = server.do_event(Event()).body["outputs"]
        assert [len(o) for o in outputs] == [4, 4, 4]
    finally:
        server.shutdown()
