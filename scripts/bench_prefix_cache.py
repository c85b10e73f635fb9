#!/usr/bin/env python3
# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""Prefix-cache measurements at llama-3-8b geometry (L=32, Hkv=8,
D=128, Smax=2048).  Needs a GPU; there is no CPU fallback.

(a) block copy alone: ONE ops.kv_block_copy gathering n = 32 and 256
    pool blocks into 8 cache slots, against the per-layer torch indexing
    that does the same job (per layer one index_put for K and one for V
    through a [B, Hkv, Smax/32, 32, D] view of the cache).  Same data,
    results compared bit for bit before timing.
(b) admission of 8 prompts of 1024 shared + 64 distinct tokens:
    prefill_cached warm (the shared prefix is in the pool, the distinct
    ends are not: gather + suffix pass + scatter of the new blocks),
    prefill_cached cold (empty pool: whole pass + scatter of every
    block) and prefill_packed on an engine without the cache.  The pool
    is put into its state before each timed call, outside the timing.
    Logits are compared before timing.

Timing: (a) hip events around `--iters` back-to-back calls; (b) a host
clock around the call plus a device synchronise, because the host-side
index work is part of what an admission costs.  The variants alternate
inside each of `--rounds` rounds in one process, after warm-up of every
variant; the median and the min over rounds are reported.

  python scripts/bench_prefix_cache.py [--layers N] [--rounds R]
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

BT = ops.KV_BLOCK_TOKENS
DEVICE = "cuda:0"


def summarize(samples: dict) -> dict:
    return {name: {"median_us": round(statistics.median(vals), 1),
                   "min_us": round(min(vals), 1)}
            for name, vals in samples.items()}


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
    """us per call, host clock + synchronise.  fns maps a name to
    (prepare, call): prepare runs outside the timing."""
    for prepare, call in fns.values():
        for _ in range(2):
            prepare()
            call()
    torch.cuda.synchronize()
    samples = {name: [] for name in fns}
    for _ in range(rounds):
        for name, (prepare, call) in fns.items():
            prepare()
            torch.cuda.synchronize()
            start = time.perf_counter()
            call()
            torch.cuda.synchronize()
            samples[name].append((time.perf_counter() - start) * 1e6)
    return samples


def bench_copy(cfg: LlamaConfig, B: int, n: int, rounds: int,
               iters: int) -> dict:
    Lr, hkv, d, smax = (cfg.num_layers, cfg.num_kv_heads, cfg.head_dim,
                        cfg.max_seq_len)
    assert smax % BT == 0 and n <= B * (smax // BT)
    gen = torch.Generator(device=DEVICE).manual_seed(n)
    bf16 = dict(dtype=torch.bfloat16, device=DEVICE)
    pool_k = torch.randn(Lr, n, hkv, BT, d, generator=gen, **bf16)
    pool_v = torch.randn(Lr, n, hkv, BT, d, generator=gen, **bf16)
    caches = [torch.zeros(Lr, B, hkv, smax, d, **bf16) for _ in range(4)]
    ours_k, ours_v, torch_k, torch_v = caches
    # block i of the pool -> slot i % B, block i // B: what a group of
    # B requests with n / B cached blocks each gathers
    ids = torch.arange(n, dtype=torch.int32, device=DEVICE)
    slot = ids % B
    blk = ids // B
    zero = torch.zeros_like(ids)
    ids_l, slot_l, blk_l = ids.long(), slot.long(), blk.long()

    def ours():
        ops.kv_block_copy(pool_k, pool_v, ours_k, ours_v, ids, zero, slot,
                          blk)

    def indexing():
        for li in range(Lr):
            torch_k[li].view(B, hkv, smax // BT, BT, d)[
                slot_l, :, blk_l] = pool_k[li, ids_l]
            torch_v[li].view(B, hkv, smax // BT, BT, d)[
                slot_l, :, blk_l] = pool_v[li, ids_l]

    ours()
    indexing()
    torch.cuda.synchronize()
    equal = bool(torch.equal(ours_k.view(torch.int16),
                             torch_k.view(torch.int16)) and
                 torch.equal(ours_v.view(torch.int16),
                             torch_v.view(torch.int16)))
    assert equal and bool(ours_k.any()), "kernel and indexing disagree"
    stats = summarize(time_rounds_events(
        {"kv_block_copy": ours, "torch_indexing": indexing}, rounds, iters))
    moved = 2 * 2 * n * Lr * hkv * BT * d * 2   # K+V, read+write, bytes
    for entry in stats.values():
        entry["GBps"] = round(moved / entry["median_us"] / 1e3, 1)
    return {"bench": "block_copy", "blocks": n, "layers": Lr, "Hkv": hkv,
            "D": d, "Smax": smax, "B": B, "bit_equal": equal,
            "MB_moved": round(moved / 2 ** 20, 1),
            "indexing_over_ours": round(
                stats["torch_indexing"]["median_us"] /
                stats["kv_block_copy"]["median_us"], 2),
            **stats}


def bench_admission(cfg: LlamaConfig, n: int, shared: int, distinct: int,
                    rounds: int) -> dict:
    blocks = (shared + distinct) // BT + n * (distinct // BT + 1) + 8
    cached = LlamaDecodeEngine(cfg, n, device=DEVICE, use_graph=False,
                               prefix_cache_blocks=blocks)
    plain = LlamaDecodeEngine(cfg, n, device=DEVICE, use_graph=False,
                              weights=cached.weights)
    gen = torch.Generator().manual_seed(1)

    def draw(count):
        return torch.randint(0, cfg.vocab_size, (count,),
                             generator=gen).tolist()
    prefix = draw(shared)
    prompts = [prefix + draw(distinct) for _ in range(n)]
    slots = list(range(n))
    primer = prefix + [0]

    def empty_pool():
        cached.clear_prefix_cache()

    def pool_with_prefix():
        cached.clear_prefix_cache()
        cached.prefill_cached([primer], [0])

    def through_cache():
        return cached.prefill_cached(prompts, slots)

    def packed():
        return plain.prefill_packed(prompts, slots)

    want = packed().float()
    empty_pool()
    cold_diff = (through_cache().float() - want).abs().max().item()
    pool_with_prefix()
    before = cached.prefix_stats["hit_tokens"]
    warm_diff = (through_cache().float() - want).abs().max().item()
    hit = cached.prefix_stats["hit_tokens"] - before
    assert hit == n * (shared // BT) * BT, hit
    stats = summarize(time_rounds_host(
        {"prefill_cached_warm": (pool_with_prefix, through_cache),
         "prefill_cached_cold": (empty_pool, through_cache),
         "prefill_packed": (lambda: None, packed)}, rounds))
    return {"bench": "admission", "config": cfg.name,
            "layers": cfg.num_layers, "prompts": n, "shared": shared,
            "distinct": distinct, "hit_tokens_warm": hit,
            "pool_blocks": blocks,
            "max_abs_logit_diff_cold": round(cold_diff, 4),
            "max_abs_logit_diff_warm": round(warm_diff, 4),
            "packed_over_warm": round(
                stats["prefill_packed"]["median_us"] /
                stats["prefill_cached_warm"]["median_us"], 3),
            "cold_over_packed": round(
                stats["prefill_cached_cold"]["median_us"] /
                stats["prefill_packed"]["median_us"], 3),
            **stats}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--layers", type=int, default=None,
                        help="override the layer count (quicker runs)")
    parser.add_argument("--rounds", type=int, default=9)
    parser.add_argument("--iters", type=int, default=10)
    parser.add_argument("--prompts", type=int, default=8)
    parser.add_argument("--shared", type=int, default=1024)
    parser.add_argument("--distinct", type=int, default=64)
    parser.add_argument("--skip-admission", action="store_true")
    args = parser.parse_args()
    assert torch.cuda.is_available(), "bench_prefix_cache.py needs a GPU"
    assert ops.HAVE_HIP_OPS, "_hip_ops extension not built"

    over = {} if args.layers is None else {"num_layers": args.layers}
    cfg = LlamaConfig.llama3_8b(**over)
    for n in (32, 256):
        print(json.dumps(bench_copy(cfg, args.prompts, n, args.rounds,
                                    args.iters)), flush=True)
    if args.skip_admission:
        return
    torch.cuda.empty_cache()
    print(json.dumps(bench_admission(cfg, args.prompts, args.shared,
                                     args.distinct, args.rounds)),
          flush=True)


if __name__ == "__main__":
    main()
