# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""Segmented multi-LoRA prefill (ops.lora_sgmv_*, lora_prefill="sgmv")
without a GPU: the host tile table, the argument checks, the CPU
reference branch, and the engine and server switch.  The cases and
helpers here are shared with test_lora_sgmv_gpu.py."""

import pytest
import torch

from mlrun_amd import ops
from mlrun_amd.models.llama import LlamaConfig, LlamaDecodeEngine
from test_lora import (MERGED_BOUND, REQUESTS, _ask, _lora_server,
                       make_adapter, merge_adapter, save_adapters)

# two prompts merging into 17 rows (a full tile and a 1-row tail), a
# skipped base segment, a 5-row tile, two full tiles and a tail; adapter
# slot 3 is named by nothing
COUNTS, IDS, NA, T = (1, 16, 17, 5, 33), (0, 0, -1, 2, 1), 4, 72
TILES = [(0, 16, 0), (16, 1, 0), (34, 5, 2), (39, 16, 1), (55, 16, 1),
         (71, 1, 1)]
RANKS = (8, 16, 32, 64)


def covered(tiles=TILES):
    return [r for r0, n, _ in tiles for r in range(r0, r0 + n)]


def int_case(R, K, N, seed=0):
    """Small-integer operands with |t| <= 32 K < 2^16 and every sum
    below 2^24: shrink is exact, and expand is the integer result rounded
    to bf16 once."""
    gen = torch.Generator().manual_seed(seed)

    def ints(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=gen)

    x, A = ints(-8, 8, T, K), ints(-4, 4, NA, R, K)
    Bm, y0 = ints(-1, 1, NA, N, R), ints(-100, 100, T, N)
    t_exp, y_exp = torch.zeros(T, R, dtype=torch.int64), y0.clone()
    for r0, n, a in TILES:
        t_exp[r0:r0 + n] = x[r0:r0 + n] @ A[a].t()
        y_exp[r0:r0 + n] += t_exp[r0:r0 + n] @ Bm[a].t()
    bf16 = torch.bfloat16
    return dict(x=x.to(bf16), A=A.to(bf16), Bm=Bm.to(bf16), y0=y0.to(bf16),
                t_exp=t_exp.float(), y_exp=y_exp.float().to(bf16))


def test_tile_table():
    tiles = ops.lora_sgmv_tiles(COUNTS, IDS)
    assert tiles.dtype == torch.int32 and tiles.tolist() == \
        [list(row) for row in TILES]
    empty = ops.lora_sgmv_tiles(COUNTS, [-1] * 5)
    assert tuple(empty.shape) == (0, 3)
    case = int_case(8, 32, 8)
    t = torch.full((T, 8), 2.5)
    assert (ops.lora_sgmv_shrink(case["x"], case["A"], empty, out=t)
            == 2.5).all()
    y = ops.lora_sgmv_expand(case["y0"].clone(), t, case["Bm"], empty)
    assert torch.equal(y, case["y0"])


@pytest.mark.parametrize("R", RANKS)
def test_cpu_reference_integer_exact(R):
    case, tiles = int_case(R, 160, 264), ops.lora_sgmv_tiles(COUNTS, IDS)
    t = ops.lora_sgmv_shrink(case["x"], case["A"], tiles,
                             out=torch.full((T, R), 7.5))
    rows = covered()
    assert torch.equal(t[rows], case["t_exp"][rows])
    assert (t[17:34] == 7.5).all()
    y = ops.lora_sgmv_expand(case["y0"].clone(), t, case["Bm"], tiles)
    assert torch.equal(y, case["y_exp"])


def test_value_errors():
    case, tiles = int_case(8, 32, 8), ops.lora_sgmv_tiles(COUNTS, IDS)
    x, A, Bm, y = case["x"], case["A"], case["Bm"], case["y0"]
    t = torch.zeros(T, 8)
    bad = [
        lambda: ops.lora_sgmv_shrink(x, A[:, :4], tiles),           # R = 4
        lambda: ops.lora_sgmv_shrink(x[:, :16].contiguous(),
                                     A[:, :, :16].contiguous(), tiles),
        lambda: ops.lora_sgmv_expand(y[:, :4].contiguous(), t,
                                     Bm[:, :4].contiguous(), tiles),
        lambda: ops.lora_sgmv_shrink(x.float(), A, tiles),
        lambda: ops.lora_sgmv_expand(y, t.double(), Bm, tiles),
        lambda: ops.lora_sgmv_expand(y.repeat(1, 2)[:, :8], t, Bm, tiles),
        lambda: ops.lora_sgmv_shrink(x, A, tiles[:, :2].contiguous()),
        lambda: ops.lora_sgmv_expand(y, t, Bm, tiles.long()),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {i} raised nothing")


# -------------------------------------------------------------- engine

ENGINE_PROMPTS = [[5, 9, 2, 77, 130], list(range(40, 61)), [7, 7, 21],
                  list(range(100, 117))]   # 5 + 21 + 3 + 17 tokens
ENGINE_IDS = [0, -1, 1, 0]


def check_engine_sgmv(device, cfg=None):
    """Engines on shared weights and tables under both ``lora_prefill``
    values, prefill_packed with ids (0, -1, 1, 0): the logits agree
    within MERGED_BOUND, the sgmv engine matches merged weights (the
    recipe of test_lora.check_parity), and an all-base call is bit-equal
    to an adapter-free engine.  Returns the measured differences."""
    cfg = cfg or LlamaConfig.tiny()
    gen = torch.Generator().manual_seed(7)
    lib = LlamaDecodeEngine(cfg, 4, device=device, use_graph=False,
                            max_adapters=2, lora_rank=8)
    for slot in (0, 1):
        lib.load_adapter(slot, make_adapter(lib.weights, 8, gen))
    sgmv = LlamaDecodeEngine(cfg, 4, device=device, use_graph=False,
                             weights=lib.weights, lora=lib.lora,
                             lora_prefill="sgmv")
    plain = LlamaDecodeEngine(cfg, 4, device=device, use_graph=False,
                              weights=lib.weights)
    slots = [0, 1, 2, 3]

    def run(engine, ids):
        engine.reset()
        kwargs = {} if ids is None else {"adapters": ids}
        return engine.prefill_packed(ENGINE_PROMPTS, slots,
                                     **kwargs).float().cpu()

    figures = {"paths": (run(sgmv, ENGINE_IDS) -
                         run(lib, ENGINE_IDS)).abs().max().item()}
    assert figures["paths"] <= MERGED_BOUND, figures
    assert torch.equal(run(sgmv, [-1] * 4), run(plain, None))
    base = run(plain, None)
    for slot in (0, 1):
        got = run(sgmv, [slot] * 4)
        merged = LlamaDecodeEngine(cfg, 4, device=device, use_graph=False)
        merge_adapter(merged, lib, slot)
        err = (got - run(merged, None)).abs().max().item()
        moved = (got - base).abs().max().item()
        figures[f"merged{slot}"] = (err, moved)
        assert err <= MERGED_BOUND and moved >= 20 * MERGED_BOUND, figures
    print("sgmv engine:", figures)
    return figures


def test_engine_cpu():
    check_engine_sgmv("cpu")
    with pytest.raises(ValueError, match="lora_prefill"):
        LlamaDecodeEngine(LlamaConfig.tiny(), 1, device="cpu",
                          lora_prefill="triton")


def test_server_round_trip(tmp_path):
    adapters, outputs = save_adapters(tmp_path), {}
    for mode in ("library", "sgmv"):
        server = _lora_server(adapters, scheduling="continuous",
                              prefill="packed", lora_prefill=mode)
        try:
            assert server.engines[0].lora_prefill == mode
            outputs[mode] = [_ask(server, prompts, name)
                             for prompts, name in REQUESTS]
        finally:
            server.shutdown()
    assert outputs["sgmv"] == outputs["library"]
    assert outputs["sgmv"][0] != outputs["sgmv"][3]   # the adapters matter
