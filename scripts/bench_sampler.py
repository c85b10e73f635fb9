#!/usr/bin/env python3
# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""Sampler measurements at the llama-3-8b vocabulary, B=32.  Needs a
GPU; there is no CPU fallback.

(a) the kernel alone: ops.sample_tokens on one [B, 128256] bf16 logits
    tensor with every row greedy, plain temperature, top_k=50,
    top_p=0.9 and all filters on, next to the engine-wide torch path
    (LlamaDecodeEngine._select_tokens) on the same logits: greedy,
    temperature=0.8, and temperature=0.8 with top_k=50.  The kernel's
    kept counts are compared with the CPU reference before timing.
(b) the graph-replayed decode step at B=32 in four engines that share
    one set of weights: sampling="engine" greedy, temperature=-1
    (per-slot temperatures on the torch path), sampling="request" with
    all rows greedy, and sampling="request" with all rows sampled
    (temperature 0.8, top_p 0.9).

Timing: (a) hip events around `--iters` back-to-back calls after a
warm-up of every variant; (b) a host clock around `--iters` replays that
end in a device synchronise.  Variants alternate inside each of
`--rounds` rounds in one process; the median, min and max over rounds
are reported.

  python scripts/bench_sampler.py [--layers N] [--skip-kernels|--skip-engine]
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

DEVICE = "cuda:0"
VOCAB = 128256
# (temperature, top_k, top_p, min_p) of every row
KERNEL_SETTINGS = {
    "greedy": (0.0, 0, 1.0, 0.0),
    "temperature": (0.8, 0, 1.0, 0.0),
    "top_k50": (0.8, 50, 1.0, 0.0),
    "top_p0.9": (0.8, 0, 0.9, 0.0),
    "all_filters": (0.8, 50, 0.9, 0.05),
}


def time_rounds(fns: dict, rounds: int, iters: int, events: bool) -> dict:
    """us per call for each fn: variants alternate within a round."""
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            if events:
                start = torch.cuda.Event(enable_timing=True)
                stop = torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(iters):
                    fn()
                stop.record()
                stop.synchronize()
                samples[name].append(
                    start.elapsed_time(stop) * 1e3 / iters)
            else:
                torch.cuda.synchronize()
                begin = time.perf_counter()
                for _ in range(iters):
                    fn()
                torch.cuda.synchronize()
                samples[name].append(
                    (time.perf_counter() - begin) * 1e6 / iters)
    return {name: {"median_us": round(statistics.median(vals), 1),
                   "min_us": round(min(vals), 1),
                   "max_us": round(max(vals), 1)}
            for name, vals in samples.items()}


def bench_kernel(B: int, rounds: int, iters: int) -> dict:
    gen = torch.Generator().manual_seed(7)
    logits = (torch.randn(B, VOCAB, generator=gen) * 3).to(torch.bfloat16)
    pos = torch.arange(B, dtype=torch.int32) + 100
    seed = torch.arange(B, dtype=torch.int64) + 1
    logits_d = logits.to(DEVICE)
    tokens = torch.zeros(B, dtype=torch.int64, device=DEVICE)
    logprob = torch.zeros(B, device=DEVICE)
    kept = torch.zeros(B, dtype=torch.int32, device=DEVICE)
    fns, kept_ok = {}, {}
    for name, (T, k, p, mp) in KERNEL_SETTINGS.items():
        host = (pos, torch.full((B,), T), torch.full((B,), k,
                                                     dtype=torch.int32),
                torch.full((B,), p), torch.full((B,), mp), seed)
        dev = [t.to(DEVICE) for t in host]
        ops.sample_tokens(logits_d, *dev, tokens, logprob, kept)
        ref = ops.sample_tokens_reference(logits, *host)
        kept_ok[name] = kept.cpu().tolist() == ref["kept"].tolist()
        fns[f"kernel_{name}"] = (lambda dev=dev: ops.sample_tokens(
            logits_d, *dev, tokens, logprob, kept))
    # the engine-wide torch path on the same logits (1 layer: only
    # _select_tokens is used)
    cfg = LlamaConfig.llama3_8b(num_layers=1)
    weights = None
    for name, kwargs in (("greedy", {}),
                         ("temperature", {"temperature": 0.8}),
                         ("top_k50", {"temperature": 0.8, "top_k": 50})):
        engine = LlamaDecodeEngine(cfg, B, device=DEVICE, use_graph=False,
                                   weights=weights, **kwargs)
        weights = engine.weights
        fns[f"torch_{name}"] = (lambda engine=engine: engine._select_tokens(
            logits_d, out=tokens))
    stats = time_rounds(fns, rounds, iters, events=True)
    return {"bench": "sampler_kernel", "B": B, "V": VOCAB,
            "kept_equals_cpu_reference": kept_ok, **stats}


def bench_engine(cfg: LlamaConfig, B: int, ctx: int, rounds: int,
                 iters: int) -> dict:
    plain = LlamaDecodeEngine(cfg, B, device=DEVICE, use_graph=True)
    shared = dict(device=DEVICE, use_graph=True, weights=plain.weights)
    per_slot = LlamaDecodeEngine(cfg, B, temperature=-1, **shared)
    per_slot.buf_temp.fill_(0.8)
    greedy = LlamaDecodeEngine(cfg, B, sampling="request", **shared)
    sampled = LlamaDecodeEngine(cfg, B, sampling="request", **shared)
    for slot in range(B):
        sampled.set_sampling(slot, temperature=0.8, top_p=0.9,
                             seed=slot + 1)
    gen = torch.Generator().manual_seed(1)
    prompts = torch.randint(0, cfg.vocab_size, (B, 16), generator=gen)
    engines = {"a_engine_greedy": plain, "b_temperature_-1": per_slot,
               "c_request_greedy": greedy, "d_request_top_p": sampled}
    for engine in engines.values():
        logits = engine.prefill(prompts)
        if engine.sampling != "request":
            engine.buf_tokens.copy_(logits.argmax(dim=-1))
        engine.capture_graph()
    # request-greedy computes the plain engine's tokens
    plain.decode_step()
    greedy.decode_step()
    torch.cuda.synchronize()
    same = torch.equal(plain.buf_tokens, greedy.buf_tokens)

    def step(engine):
        def run():
            engine.cache_lens.fill_(ctx)
            engine.decode_step()
        return run

    stats = time_rounds({name: step(engine)
                         for name, engine in engines.items()},
                        rounds, iters, events=False)
    base = stats["a_engine_greedy"]["median_us"]
    return {"bench": "decode_step_graph", "config": cfg.name,
            "layers": cfg.num_layers, "B": B, "ctx": ctx,
            "request_greedy_tokens_equal_engine_greedy": same,
            **{f"{name[:1]}_over_a": round(
                stats[name]["median_us"] / base, 4)
               for name in list(engines)[1:]},
            **stats}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--layers", type=int, default=None,
                        help="override the layer count (quicker runs)")
    parser.add_argument("--batch", type=int, default=32)
    parser.add_argument("--ctx", type=int, default=160)
    parser.add_argument("--rounds", type=int, default=15)
    parser.add_argument("--iters", type=int, default=20)
    parser.add_argument("--skip-kernels", action="store_true")
    parser.add_argument("--skip-engine", action="store_true")
    args = parser.parse_args()
    assert torch.cuda.is_available(), "bench_sampler.py needs a GPU"
    assert ops.HAVE_HIP_OPS, "_hip_ops extension not built"

    if not args.skip_kernels:
        print(json.dumps(bench_kernel(args.batch, args.rounds, args.iters)),
              flush=True)
    if args.skip_engine:
        return
    over = {} if args.layers is None else {"num_layers": args.layers}
    cfg = LlamaConfig.llama3_8b(**over)
    print(json.dumps(bench_engine(cfg, args.batch, args.ctx, args.rounds,
                                  args.iters)), flush=True)


if __name__ == "__main__":
    main()
