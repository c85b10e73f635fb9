#!/usr/bin/env python3
# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""Multi-LoRA measurements at llama-3-8b shapes.  Needs a GPU; there is
no CPU fallback.

(a) kernels alone: ops.lora_shrink and ops.lora_expand at the four
    projection shapes (qkv, attn-out, gate|up, down), B=32, table rank
    16 and 64, rows spread over 1, 4 or 32 distinct adapters, plus the
    all-base case (every id -1: what an enabled engine pays for rows
    without an adapter).  Outputs are compared with the CPU reference
    of the same op before timing.
(b) the graph-replayed decode step at B=32 in three settings that share
    one set of weights: max_adapters=0, adapters enabled with every id
    -1, adapters enabled with every row adapted (4 adapters, rank 16).

Timing: (a) hip events around `--iters` back-to-back calls after a
warm-up of every variant; (b) a host clock around `--iters` replays that
end in a device synchronise.  Variants alternate inside each of
`--rounds` rounds in one process; median and min over rounds are
reported, and for (b) the spread of the rounds as well.

  python scripts/bench_lora.py [--layers N] [--skip-kernels|--skip-engine]
"""

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(
    __file__))))

import torch  # noqa: E402

from mlrun_amd import ops  # noqa: E402
from mlrun_amd.models.llama import (LORA_PROJECTIONS,  # noqa: E402
                                    LlamaConfig, LlamaDecodeEngine)

DEVICE = "cuda:0"
# llama-3-8b projections: name -> (N, K)
SHAPES = {"wqkv": (6144, 4096), "wo": (4096, 4096),
          "wgu": (28672, 4096), "wdown": (4096, 14336)}
NA = 32


def time_rounds_events(fns: dict, rounds: int, iters: int) -> dict:
    """us per call for each fn: variants alternate within a round."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            start = torch.cuda.Event(enable_timing=True)
            stop = torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(iters):
                fn()
            stop.record()
            stop.synchronize()
            samples[name].append(start.elapsed_time(stop) * 1e3 / iters)
    return samples


def time_rounds_host(fns: dict, rounds: int, iters: int,
                     warmup: int = 5) -> dict:
    """us per call, host clock + synchronise."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            start = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            samples[name].append(
                (time.perf_counter() - start) * 1e6 / iters)
    return samples


def summarize(samples: dict, spread: bool = False) -> dict:
    out = {}
    for name, vals in samples.items():
        out[name] = {"median_us": round(statistics.median(vals), 1),
                     "min_us": round(min(vals), 1)}
        if spread:
            out[name]["max_us"] = round(max(vals), 1)
    return out


def bench_kernels(B: int, R: int, rounds: int, iters: int) -> list:
    rows = []
    gen = torch.Generator().manual_seed(R)
    for proj, (N, K) in SHAPES.items():
        x = torch.randn(B, K, generator=gen).to(torch.bfloat16)
        y0 = torch.randn(B, N, generator=gen).to(torch.bfloat16)
        A = (torch.randn(NA, R, K, generator=gen) * 0.05
             ).to(torch.bfloat16)
        Bm = (torch.randn(NA, N, R, generator=gen) * 0.1
              ).to(torch.bfloat16)
        ids = {"distinct1": torch.zeros(B, dtype=torch.int32),
               "distinct4": (torch.arange(B) % 4).to(torch.int32),
               "distinct32": (torch.arange(B) % NA).to(torch.int32),
               "all_base": torch.full((B,), -1, dtype=torch.int32)}
        # same numbers as the CPU reference, before any timing
        t_ref = ops.lora_shrink(x, A, ids["distinct32"])
        y_ref = ops.lora_expand(y0.clone(), t_ref, Bm, ids["distinct32"])
        xd, yd, Ad, Bd = x.to(DEVICE), y0.to(DEVICE), A.to(DEVICE), \
            Bm.to(DEVICE)
        idd = {name: v.to(DEVICE) for name, v in ids.items()}
        t = torch.zeros(B, R, device=DEVICE)
        ops.lora_shrink(xd, Ad, idd["distinct32"], out=t)
        y = ops.lora_expand(yd.clone(), t, Bd, idd["distinct32"])
        t_diff = (t.cpu() - t_ref).abs().max().item()
        y_diff = (y.cpu().float() - y_ref.float()).abs().max().item()

        fns = {}
        for name, idx in idd.items():
            fns[f"shrink_{name}"] = (
                lambda idx=idx: ops.lora_shrink(xd, Ad, idx, out=t))
            # the timed expand keeps adding to yd: values grow, the
            # work per call does not change
            fns[f"expand_{name}"] = (
                lambda idx=idx: ops.lora_expand(yd, t, Bd, idx))
        stats = summarize(time_rounds_events(fns, rounds, iters))
        # bytes the pair has to read with 32 distinct adapters
        shrink_bytes = B * R * K * 2 + B * K * 2
        expand_bytes = B * N * R * 2 + 2 * B * N * 2
        rows.append({
            "bench": "lora_kernels", "proj": proj, "N": N, "K": K,
            "B": B, "R": R, "NA": NA,
            "max_abs_t_diff_vs_cpu": round(t_diff, 6),
            "max_abs_y_diff_vs_cpu": round(y_diff, 4),
            "shrink_distinct32_GBps": round(
                shrink_bytes / stats["shrink_distinct32"]["median_us"]
                / 1e3, 1),
            "expand_distinct32_GBps": round(
                expand_bytes / stats["expand_distinct32"]["median_us"]
                / 1e3, 1),
            **stats})
    return rows


def bench_engine(cfg: LlamaConfig, B: int, ctx: int, rank: int,
                 n_adapters: int, rounds: int, iters: int) -> dict:
    plain = LlamaDecodeEngine(cfg, B, device=DEVICE, use_graph=True)
    idle = LlamaDecodeEngine(cfg, B, device=DEVICE, use_graph=True,
                             weights=plain.weights,
                             max_adapters=n_adapters, lora_rank=rank)
    busy = LlamaDecodeEngine(cfg, B, device=DEVICE, use_graph=True,
                             weights=plain.weights, lora=idle.lora)
    # random tables: the values do not change the work
    for tables in idle.lora.layers:
        for proj in LORA_PROJECTIONS:
            a_tab, b_tab = tables[proj]
            a_tab.normal_(0.0, 0.02)
            b_tab.normal_(0.0, 0.02)
    gen = torch.Generator().manual_seed(1)
    prompts = torch.randint(0, cfg.vocab_size, (B, 16), generator=gen)
    busy_ids = [b % n_adapters for b in range(B)]
    for engine, ids in ((plain, None), (idle, None), (busy, busy_ids)):
        kwargs = {} if ids is None else {"adapters": ids}
        logits = engine.prefill(prompts, **kwargs)
        engine.buf_tokens.copy_(logits.argmax(dim=-1))
        engine.capture_graph()
    assert idle.buf_adapter.tolist() == [-1] * B
    assert busy.buf_adapter.tolist() == busy_ids
    # enabled with every id -1 computes the plain engine's step, except
    # that qkv is rounded to bf16 before rope (no slab-fused consumer)
    plain.decode_step()
    idle.decode_step()
    busy.decode_step()
    torch.cuda.synchronize()
    idle_diff = (idle.buf_logits.float() - plain.buf_logits.float()
                 ).abs().max().item()
    busy_diff = (busy.buf_logits.float() - plain.buf_logits.float()
                 ).abs().max().item()

    def step(engine):
        def run():
            engine.cache_lens.fill_(ctx)
            engine.decode_step()
        return run

    samples = time_rounds_host(
        {"a_max_adapters_0": step(plain), "b_enabled_all_base": step(idle),
         "c_enabled_all_adapted": step(busy)}, rounds, iters)
    stats = summarize(samples, spread=True)
    base = stats["a_max_adapters_0"]["median_us"]
    return {"bench": "decode_step_graph", "config": cfg.name,
            "layers": cfg.num_layers, "B": B, "ctx": ctx, "rank": rank,
            "adapters": n_adapters,
            "max_abs_logit_diff_b_vs_a": round(idle_diff, 4),
            "max_abs_logit_diff_c_vs_a": round(busy_diff, 4),
            "b_over_a": round(
                stats["b_enabled_all_base"]["median_us"] / base, 4),
            "c_over_a": round(
                stats["c_enabled_all_adapted"]["median_us"] / base, 4),
            **stats}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--layers", type=int, default=None,
                        help="override the layer count (quicker runs)")
    parser.add_argument("--batch", type=int, default=32)
    parser.add_argument("--ctx", type=int, default=160)
    parser.add_argument("--rank", type=int, default=16)
    parser.add_argument("--adapters", type=int, default=4)
    parser.add_argument("--rounds", type=int, default=15)
    parser.add_argument("--iters", type=int, default=20)
    parser.add_argument("--skip-kernels", action="store_true")
    parser.add_argument("--skip-engine", action="store_true")
    args = parser.parse_args()
    assert torch.cuda.is_available(), "bench_lora.py needs a GPU"
    assert ops.HAVE_HIP_OPS, "_hip_ops extension not built"

    for rank in () if args.skip_kernels else (16, 64):
        for row in bench_kernels(args.batch, rank, args.rounds,
                                 args.iters):
            print(json.dumps(row), flush=True)
    if args.skip_engine:
        return
    over = {} if args.layers is None else {"num_layers": args.layers}
    cfg = LlamaConfig.llama3_8b(**over)
    print(json.dumps(bench_engine(cfg, args.batch, args.ctx, args.rank,
                                  args.adapters, args.rounds, args.iters)),
          flush=True)


if __name__ == "__main__":
    main()
