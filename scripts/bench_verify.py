#!/usr/bin/env python3
# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""Speculative-decoding measurements at llama-3-8b head geometry
(Hq=32, Hkv=8, D=128).  Needs a GPU; there is no CPU fallback.

(a) verify attention alone: ops.attn_verify vs ops.attn_prefill on the
    SAME inputs (the only way to compute it before attn_verify) and vs
    QL calls of ops.attn_decode, B=32, QL=4, contexts 160/1024/4096;
    attn_verify also at forced split counts.  Outputs are compared
    before timing.
(b) engine step: verify_step(k=3) (eager) vs the graph-replayed
    decode_step at B=32.  Their ratio is the break-even mean number of
    tokens a verify step has to emit.
(c) end to end: generate vs generate_speculative on the same
    random-init model and prompts, with the observed acceptance.

Timing: (a) hip events around `--iters` back-to-back calls after
warm-up of every variant; (b) and (c) a host clock around work that
ends in a device synchronise, because the eager verify pass and the
per-step length read are host work that a user pays for.  Variants
alternate inside each of `--rounds` rounds in one process; median and
min over rounds are reported.

  python scripts/bench_verify.py [--config llama-3-8b] [--layers N]
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


def time_rounds_host(fns: dict, rounds: int, iters: int = 1,
                     warmup: int = 2) -> dict:
    """us per call, host clock + synchronise (host work included)."""
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


def summarize(samples: dict) -> dict:
    return {name: {"median_us": round(statistics.median(vals), 1),
                   "min_us": round(min(vals), 1)}
            for name, vals in samples.items()}


def bench_attention(B: int, QL: int, ctx: int, rounds: int,
                    iters: int) -> dict:
    device = "cuda:0"
    torch.manual_seed(B * 10007 + ctx)
    smax = (ctx + QL + 63) // 64 * 64
    q = torch.randn(B, QL, HQ, D, device=device, dtype=torch.bfloat16)
    kc = torch.randn(B, HKV, smax, D, device=device, dtype=torch.bfloat16)
    vc = torch.randn_like(kc)
    base = torch.full((B,), ctx, device=device, dtype=torch.int32)
    cu = torch.arange(0, (B + 1) * QL, QL, device=device,
                      dtype=torch.int32)
    slots = torch.arange(B, device=device, dtype=torch.int32)
    out = torch.empty(B * QL, HQ * D, device=device, dtype=torch.bfloat16)
    out_dec = torch.empty(B, HQ, D, device=device, dtype=torch.bfloat16)
    q_flat = q.view(B * QL, HQ, D)
    q_rows = [q[:, j].contiguous() for j in range(QL)]
    lens = [base + j + 1 for j in range(QL)]
    scale = D ** -0.5
    ns_default = ops.pick_verify_nsplit(B, HKV, smax)
    ns_decode = ops.pick_attn_nsplit(B, HKV)
    ws = torch.empty(ops.attn_verify_ws_numel(B, QL, HQ, 16),
                     device=device, dtype=torch.float32)
    ws_dec = torch.empty(B * HQ * ns_decode * (D + 2), device=device,
                         dtype=torch.float32)

    def verify(nsplit):
        return lambda: ops.attn_verify(q, kc, vc, base, scale, out=out,
                                       nsplit=nsplit, partial_ws=ws)

    def prefill():
        return ops.attn_prefill(q_flat, kc, vc, cu, slots, base, scale,
                                out=out, max_q_len=QL)

    def decode_x_ql():
        for j in range(QL):
            ops.attn_decode(q_rows[j], kc, vc, lens[j], scale,
                            out=out_dec, partial_ws=ws_dec,
                            nsplit=ns_decode)

    want = prefill().float().clone()
    diffs = {}
    fns = {"attn_verify": verify(ns_default), "attn_prefill": prefill,
           f"attn_decode_x{QL}": decode_x_ql}
    diffs["default"] = (verify(ns_default)().float() - want
                        ).abs().max().item()
    for ns in (1, 2, 4, 8, 16):
        if ns <= smax // 64:
            fns[f"attn_verify_ns{ns}"] = verify(ns)
            diffs[f"ns{ns}"] = (verify(ns)().float() - want
                                ).abs().max().item()
    stats = summarize(time_rounds_events(fns, rounds, iters))
    kv_bytes = 2.0 * B * HKV * (ctx + QL) * D * 2  # K and V, read once
    ours = stats["attn_verify"]["median_us"]
    return {"bench": "verify_attention", "B": B, "QL": QL, "ctx": ctx,
            "Hq": HQ, "Hkv": HKV, "nsplit_default": ns_default,
            "max_abs_diff_vs_attn_prefill": round(max(diffs.values()), 4),
            "attn_verify_kv_GBps": round(kv_bytes / ours / 1e3, 1),
            "prefill_over_verify": round(
                stats["attn_prefill"]["median_us"] / ours, 3),
            "decode_xQL_over_verify": round(
                stats[f"attn_decode_x{QL}"]["median_us"] / ours, 3),
            **stats}


def bench_engine(cfg: LlamaConfig, B: int, S: int, k: int, max_new: int,
                 rounds: int) -> list:
    plain = LlamaDecodeEngine(cfg, B, device="cuda:0", use_graph=True)
    spec = LlamaDecodeEngine(cfg, B, device="cuda:0", use_graph=False,
                             weights=plain.weights)
    gen = torch.Generator().manual_seed(1)
    prompts = torch.randint(0, cfg.vocab_size, (B, S), generator=gen)
    plain.buf_tokens.copy_(plain.prefill(prompts).argmax(dim=-1))
    spec.buf_tokens.copy_(spec.prefill(prompts).argmax(dim=-1))
    plain.capture_graph()
    drafts = torch.randint(0, cfg.vocab_size, (B, k), generator=gen
                           ).to(spec.device)

    # same token at the same position through both paths: row 0 of the
    # verify pass against the decode step's logits
    plain.decode_step()
    spec.verify_step(drafts)
    logit_diff = (spec.buf_verify_logits[:, 0].float() -
                  plain.buf_logits.float()).abs().max().item()

    # (b) one step each at a fixed context of S cached tokens
    def decode_step():
        plain.cache_lens.fill_(S)
        plain.decode_step()

    def verify_step():
        spec.cache_lens.fill_(S)
        spec.verify_step(drafts)

    step = summarize(time_rounds_host(
        {"decode_step_graph": decode_step, "verify_step_eager": verify_step},
        rounds, iters=10, warmup=5))
    ratio = step["verify_step_eager"]["median_us"] / \
        step["decode_step_graph"]["median_us"]
    results = [{"bench": "engine_step", "config": cfg.name,
                "layers": cfg.num_layers, "B": B, "ctx": S, "k": k,
                "break_even_tokens_per_verify_step": round(ratio, 2),
                "max_abs_logit_diff_vs_decode_step": round(logit_diff, 4),
                **step}]

    # (c) whole generations, same prompts
    outs = {}

    def run_plain():
        outs["plain"] = plain.generate(prompts, max_new)

    def run_spec():
        outs["spec"] = spec.generate_speculative(prompts, max_new, k=k)

    for key in spec.spec_stats:
        spec.spec_stats[key] = 0
    e2e = summarize(time_rounds_host(
        {"generate": run_plain, "generate_speculative": run_spec},
        max(rounds // 3, 3), warmup=1))
    stats = dict(spec.spec_stats)
    # on the GPU the two paths use different GEMMs (skinny vs library):
    # a near-tie in the logits may flip, and the rows part ways there
    same = (outs["plain"] == outs["spec"])
    agree = same.float().mean().item()
    prefix = same.long().cumprod(dim=1).sum(dim=1)  # per row
    first_split = prefix.float().mean().item()
    runs = max(rounds // 3, 3) + 1  # timed rounds + one warm-up
    # a live row emits n_accepted + 1 tokens per verify step
    row_steps = max(stats["drafted"] // k, 1)
    tokens_per_step = 1.0 + stats["accepted"] / row_steps
    results.append({
        "bench": "generate", "config": cfg.name, "layers": cfg.num_layers,
        "B": B, "prompt": S, "max_new": max_new, "k": k,
        "acceptance_rate": round(stats["accepted"] /
                                 max(stats["drafted"], 1), 4),
        "verify_steps_per_generation": round(stats["steps"] / runs, 1),
        "mean_tokens_per_row_per_verify_step": round(tokens_per_step, 3),
        "token_agreement_with_generate": round(agree, 4),
        "mean_tokens_before_first_difference": round(first_split, 1),
        "min_max_tokens_before_first_difference": [
            int(prefix.min()), int(prefix.max())],
        "speculative_over_plain_time": round(
            e2e["generate_speculative"]["median_us"] /
            e2e["generate"]["median_us"], 3),
        **e2e})
    return results


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", default="llama-3-8b",
                        choices=["llama-3-8b", "tiny"])
    parser.add_argument("--layers", type=int, default=None,
                        help="override the layer count (quicker runs)")
    parser.add_argument("--batch", type=int, default=32)
    parser.add_argument("--prompt", type=int, default=128)
    parser.add_argument("--max-new", type=int, default=64)
    parser.add_argument("--k", type=int, default=3)
    parser.add_argument("--rounds", type=int, default=15)
    parser.add_argument("--iters", type=int, default=20)
    parser.add_argument("--skip-engine", action="store_true")
    parser.add_argument("--skip-attention", action="store_true")
    args = parser.parse_args()
    assert torch.cuda.is_available(), "bench_verify.py needs a GPU"
    assert ops.HAVE_HIP_OPS, "_hip_ops extension not built"

    for ctx in () if args.skip_attention else (160, 1024, 4096):
        print(json.dumps(bench_attention(32, 4, ctx, args.rounds,
                                         args.iters)), flush=True)
    if args.skip_engine:
        return
    over = {} if args.layers is None else {"num_layers": args.layers}
    cfg = LlamaConfig.tiny(**over) if args.config == "tiny" else \
        LlamaConfig.llama3_8b(**over)
    for row in bench_engine(cfg, args.batch, args.prompt, args.k,
                            args.max_new, args.rounds):
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
