#!/usr/bin/env python3
# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""Packed-prefill measurements at llama-3-8b head geometry
(Hq=32, Hkv=8, D=128).  Needs a GPU; there is no CPU fallback.

(a) attention kernel alone: ops.attn_prefill vs
    torch scaled_dot_product_attention on equal-length causal batches
    (B x S), same random data, outputs compared before timing.
(b) admission cost: ONE engine.prefill_packed over eight prompts of
    eight distinct lengths vs the eight engine.prefill_slots calls the
    default prefill="exact" mode makes for the same prompts.

Timing: hip events around `--iters` back-to-back calls, after warm-up
of every shape; the variants alternate inside each of `--rounds`
rounds in one process and the median (and min) over rounds is
reported.  (b) is timed with a host clock around the calls plus a
device synchronise, because the host-side work per call is part of
what an admission costs.

  python scripts/bench_prefill.py [--config llama-3-8b] [--layers N]
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
from mlrun_amd.models.llama import (LlamaConfig,  # noqa: E402
                                    LlamaDecodeEngine)

HQ, HKV, D = 32, 8, 128


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


def time_rounds_host(fns: dict, rounds: int) -> dict:
    """us per call, host clock + synchronise (host work included)."""
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            start = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            samples[name].append((time.perf_counter() - start) * 1e6)
    return samples


def summarize(samples: dict) -> dict:
    return {name: {"median_us": round(statistics.median(vals), 1),
                   "min_us": round(min(vals), 1)}
            for name, vals in samples.items()}


def bench_attention(B: int, S: int, rounds: int, iters: int) -> dict:
    device = "cuda:0"
    torch.manual_seed(B * 10007 + S)
    q = torch.randn(B * S, HQ, D, device=device, dtype=torch.bfloat16)
    kc = torch.randn(B, HKV, S, D, device=device, dtype=torch.bfloat16)
    vc = torch.randn_like(kc)
    cu = torch.arange(0, (B + 1) * S, S, device=device, dtype=torch.int32)
    slots = torch.arange(B, device=device, dtype=torch.int32)
    starts = torch.zeros(B, device=device, dtype=torch.int32)
    out = torch.empty(B * S, HQ * D, device=device, dtype=torch.bfloat16)
    qh = q.view(B, S, HQ, D).transpose(1, 2).contiguous()
    scale = D ** -0.5

    def ours():
        return ops.attn_prefill(q, kc, vc, cu, slots, starts, scale,
                                out=out, max_q_len=S)

    def sdpa():
        return torch.nn.functional.scaled_dot_product_attention(
            qh, kc, vc, is_causal=True, enable_gqa=True)

    want = sdpa().transpose(1, 2).reshape(B * S, HQ * D).float()
    max_diff = (ours().float() - want).abs().max().item()
    stats = summarize(time_rounds_events(
        {"attn_prefill": ours, "sdpa": sdpa}, rounds, iters))
    flops = 4.0 * B * HQ * D * S * (S + 1) / 2  # causal QK^T + PV
    for entry in stats.values():
        entry["tflops"] = round(flops / entry["median_us"] / 1e6, 1)
    return {"bench": "attention", "B": B, "S": S, "Hq": HQ, "Hkv": HKV,
            "D": D, "max_abs_diff_vs_sdpa": round(max_diff, 4),
            "sdpa_over_ours": round(stats["sdpa"]["median_us"] /
                                    stats["attn_prefill"]["median_us"], 3),
            **stats}


def bench_admission(cfg: LlamaConfig, lengths, rounds: int) -> dict:
    engine = LlamaDecodeEngine(cfg, len(lengths), device="cuda:0",
                               use_graph=False)
    gen = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, cfg.vocab_size, (n,),
                             generator=gen).tolist() for n in lengths]
    slot_ids = list(range(len(lengths)))
    tokens = [torch.tensor([p], dtype=torch.int64) for p in prompts]
    slot_t = [torch.tensor([s], dtype=torch.long) for s in slot_ids]

    def packed():
        return engine.prefill_packed(prompts, slot_ids)

    def exact():
        return torch.cat([engine.prefill_slots(t, s)
                          for t, s in zip(tokens, slot_t)])

    max_diff = (packed().float() - exact().float()).abs().max().item()
    stats = summarize(time_rounds_host(
        {"prefill_packed_x1": packed,
         f"prefill_slots_x{len(lengths)}": exact}, rounds))
    names = list(stats)
    return {"bench": "admission", "config": cfg.name,
            "layers": cfg.num_layers, "lengths": list(lengths),
            "tokens": sum(lengths),
            "max_abs_logit_diff": round(max_diff, 4),
            "exact_over_packed": round(stats[names[1]]["median_us"] /
                                       stats[names[0]]["median_us"], 3),
            **stats}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", default="llama-3-8b",
                        choices=["llama-3-8b", "tiny"])
    parser.add_argument("--layers", type=int, default=None,
                        help="override the layer count (quicker runs)")
    parser.add_argument("--rounds", type=int, default=15)
    parser.add_argument("--iters", type=int, default=20)
    parser.add_argument("--lengths", default="24,40,56,72,88,104,120,136")
    parser.add_argument("--skip-admission", action="store_true")
    args = parser.parse_args()
    assert torch.cuda.is_available(), "bench_prefill.py needs a GPU"
    assert ops.HAVE_HIP_OPS, "_hip_ops extension not built"

    for B, S in [(8, 512), (4, 1024), (1, 2048)]:
        print(json.dumps(bench_attention(B, S, args.rounds, args.iters)),
              flush=True)
    if args.skip_admission:
        return
    over = {} if args.layers is None else {"num_layers": args.layers}
    cfg = LlamaConfig.tiny(**over) if args.config == "tiny" else \
        LlamaConfig.llama3_8b(**over)
    lengths = [int(n) for n in args.lengths.split(",")]
    print(json.dumps(bench_admission(cfg, lengths, args.rounds)),
          flush=True)


if __name__ == "__main__":
    main()
