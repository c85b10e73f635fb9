#!/usr/bin/env python3
# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""Multi-adapter prefill measurements at llama-3-8b shapes.  Needs a GPU;
there is no CPU fallback.

(a) kernels alone: ops.lora_sgmv_shrink and ops.lora_sgmv_expand at the
    four projection shapes (qkv, attn-out, gate|up, down), T = 640 rows,
    table rank 16 and 64, the rows split over 1, 4 or 8 adapters, plus
    640 rows of which one prompt in five is adapted ("sparse").  Outputs
    are compared with the CPU branch of the same op before timing.
(b) engine.prefill_packed of 640 tokens with 0, 1, 4 and 8 distinct
    adapters under lora_prefill="library" and "sgmv", and on an engine
    without adapter tables, all on one set of weights.  640 tokens are
    5 prompts of 128; 8 distinct adapters need 8 prompts, so that case
    runs 8 prompts of 80.

Timing: (a) hip events around `--iters` back-to-back calls after a
warm-up of every variant; (b) a host clock around `--iters` calls that
end in a device synchronise.  Variants alternate inside each of
`--rounds` rounds in one process; median, min and max over the rounds
are reported.

  python scripts/bench_lora_prefill.py [--layers N] [--skip-kernels|--skip-engine]
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
NA = 8
TOKENS = 640


def prompt_split(n_adapters: int):
    """(counts, ids) of the 640-token call with n_adapters distinct ids."""
    n = 8 if n_adapters > 5 else 5
    counts = [TOKENS // n] * n
    ids = [i % n_adapters if n_adapters else -1 for i in range(n)]
    return counts, ids


def time_rounds(fns: dict, rounds: int, iters: int, events: bool) -> dict:
    """us per call for each fn: variants alternate within a round."""
    for fn in fns.values():
        for _ in range(3):
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
                took = start.elapsed_time(stop) * 1e3
            else:
                torch.cuda.synchronize()
                begin = time.perf_counter()
                for _ in range(iters):
                    fn()
                torch.cuda.synchronize()
                took = (time.perf_counter() - begin) * 1e6
            samples[name].append(took / iters)
    return {name: {"median_us": round(statistics.median(vals), 1),
                   "min_us": round(min(vals), 1),
                   "max_us": round(max(vals), 1)}
            for name, vals in samples.items()}


def bench_kernels(R: int, rounds: int, iters: int) -> list:
    rows = []
    gen = torch.Generator().manual_seed(R)
    splits = {f"adapters{n}": prompt_split(n) for n in (1, 4, 8)}
    splits["sparse"] = ([128] * 5, [-1, -1, 3, -1, -1])
    for proj, (N, K) in SHAPES.items():
        x = torch.randn(TOKENS, K, generator=gen).to(torch.bfloat16)
        y0 = torch.randn(TOKENS, N, generator=gen).to(torch.bfloat16)
        A = (torch.randn(NA, R, K, generator=gen) * 0.05
             ).to(torch.bfloat16)
        Bm = (torch.randn(NA, N, R, generator=gen) * 0.1
              ).to(torch.bfloat16)
        # same numbers as the CPU branch, before any timing
        tiles = ops.lora_sgmv_tiles(*splits["adapters8"])
        t_ref = ops.lora_sgmv_shrink(x, A, tiles)
        y_ref = ops.lora_sgmv_expand(y0.clone(), t_ref, Bm, tiles)
        xd, yd, Ad, Bd = x.to(DEVICE), y0.to(DEVICE), A.to(DEVICE), \
            Bm.to(DEVICE)
        t = torch.zeros(TOKENS, R, device=DEVICE)
        ops.lora_sgmv_shrink(xd, Ad, tiles.to(DEVICE), out=t)
        y = ops.lora_sgmv_expand(yd.clone(), t, Bd, tiles.to(DEVICE))
        t_diff = (t.cpu() - t_ref).abs().max().item()
        y_diff = (y.cpu().float() - y_ref.float()).abs().max().item()

        fns = {}
        for name, (counts, ids) in splits.items():
            table = ops.lora_sgmv_tiles(counts, ids, DEVICE)
            fns[f"shrink_{name}"] = (
                lambda table=table: ops.lora_sgmv_shrink(xd, Ad, table,
                                                         out=t))
            # the timed expand keeps adding to yd: values grow, the
            # work per call does not change
            fns[f"expand_{name}"] = (
                lambda table=table: ops.lora_sgmv_expand(yd, t, Bd, table))
        stats = time_rounds(fns, rounds, iters, events=True)
        # bytes the pair has to move when every row is adapted
        shrink_bytes = TOKENS * K * 2 + NA * R * K * 2 + TOKENS * R * 4
        expand_bytes = 2 * TOKENS * N * 2 + NA * N * R * 2 + TOKENS * R * 4
        rows.append({
            "bench": "lora_sgmv_kernels", "proj": proj, "N": N, "K": K,
            "T": TOKENS, "R": R,
            "max_abs_t_diff_vs_cpu": round(t_diff, 6),
            "max_abs_y_diff_vs_cpu": round(y_diff, 4),
            "shrink_adapters8_GBps": round(
                shrink_bytes / stats["shrink_adapters8"]["median_us"] / 1e3,
                1),
            "expand_adapters8_GBps": round(
                expand_bytes / stats["expand_adapters8"]["median_us"] / 1e3,
                1),
            **stats})
    return rows


def bench_engine(cfg: LlamaConfig, rank: int, rounds: int, iters: int,
                 plain: LlamaDecodeEngine) -> list:
    lib = LlamaDecodeEngine(cfg, 8, device=DEVICE, use_graph=False,
                            weights=plain.weights, max_adapters=NA,
                            lora_rank=rank)
    sgmv = LlamaDecodeEngine(cfg, 8, device=DEVICE, use_graph=False,
                             weights=plain.weights, lora=lib.lora,
                             lora_prefill="sgmv")
    # random tables: the values do not change the work
    for tables in lib.lora.layers:
        for proj in LORA_PROJECTIONS:
            a_tab, b_tab = tables[proj]
            a_tab.normal_(0.0, 0.02)
            b_tab.normal_(0.0, 0.02)
    gen = torch.Generator().manual_seed(1)
    rows = []
    for n_adapters in (0, 1, 4, 8):
        counts, ids = prompt_split(n_adapters)
        prompts = [torch.randint(0, cfg.vocab_size, (c,),
                                 generator=gen).tolist() for c in counts]
        slots = list(range(len(counts)))

        def call(engine, adapters):
            def run():
                engine.reset()
                kwargs = {} if adapters is None else {"adapters": adapters}
                return engine.prefill_packed(prompts, slots, **kwargs)
            return run

        fns = {"no_tables": call(plain, None), "library": call(lib, ids),
               "sgmv": call(sgmv, ids)}
        diff = (fns["sgmv"]().float() - fns["library"]().float()
                ).abs().max().item()
        stats = time_rounds(fns, rounds, iters, events=False)
        base = stats["no_tables"]["median_us"]
        rows.append({
            "bench": "prefill_packed", "config": cfg.name,
            "layers": cfg.num_layers, "tokens": TOKENS,
            "prompts": len(counts), "rank": rank, "adapters": n_adapters,
            "max_abs_logit_diff_sgmv_vs_library": round(diff, 4),
            "library_over_no_tables": round(
                stats["library"]["median_us"] / base, 3),
            "sgmv_over_no_tables": round(
                stats["sgmv"]["median_us"] / base, 3),
            **stats})
    return rows


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--layers", type=int, default=None,
                        help="override the layer count (quicker runs)")
    parser.add_argument("--rounds", type=int, default=9)
    parser.add_argument("--iters", type=int, default=3)
    parser.add_argument("--kernel-iters", type=int, default=20)
    parser.add_argument("--skip-kernels", action="store_true")
    parser.add_argument("--skip-engine", action="store_true")
    args = parser.parse_args()
    assert torch.cuda.is_available(), "bench_lora_prefill.py needs a GPU"
    assert ops.HAVE_HIP_OPS, "_hip_ops extension not built"

    for rank in () if args.skip_kernels else (16, 64):
        for row in bench_kernels(rank, args.rounds, args.kernel_iters):
            print(json.dumps(row), flush=True)
    if args.skip_engine:
        return
    over = {"max_seq_len": 256}
    if args.layers is not None:
        over["num_layers"] = args.layers
    cfg = LlamaConfig.llama3_8b(**over)
    plain = LlamaDecodeEngine(cfg, 8, device=DEVICE, use_graph=False)
    for rank in (16, 64):
        for row in bench_engine(cfg, rank, args.rounds, args.iters, plain):
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
