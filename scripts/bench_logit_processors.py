#!/usr/bin/env python3
# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""Logit-processor measurements at the llama-3-8b vocabulary, B=32.
Needs a GPU; there is no CPU fallback.

(a) the kernel alone: ops.logit_processors on one [B, 128256] bf16
    logits tensor and a [B, 128256] int32 state table (5 % of the words
    non-zero) with every row neutral, every row penalised, and every row
    penalised with 64 bias entries, with and without pending tokens, and
    the penalised call again over 16 copies of logits and state taken in
    turn, so that no call finds its operands in the Infinity Cache.
    The result of each setting is compared bit for bit with the CPU
    branch before timing.  Repeated calls keep penalising the same
    logits, so the values drift to 0 / -inf; the work per call does not
    depend on them.
(b) the graph-replayed decode step at B=32 in four engines that share
    one set of weights: sampling="request" without the flag, and
    logit_processors=True with every row neutral, every row penalised,
    and every row penalised with 64 bias entries.  `--baseline-only`
    times the first engine alone (the script then runs unchanged on a
    tree without the feature, for an alternating comparison).

Timing: (a) hip events around `--iters` back-to-back calls after a
warm-up of every variant; (b) a host clock around `--iters` replays that
end in a device synchronise.  Variants alternate inside each of
`--rounds` rounds in one process; the median, min and max over rounds
are reported.

  python scripts/bench_logit_processors.py [--layers N]
      [--skip-kernels|--skip-engine] [--baseline-only]
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
COLD_SETS = 16     # x 24.6 MB of logits + state at B=32: 394 MB
PENALTIES = dict(repetition_penalty=1.2, presence_penalty=0.5,
                 frequency_penalty=0.25)


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


def bias_of(row: int, vocab: int) -> dict:
    """64 distinct ids spread over the vocabulary, row-dependent."""
    return {(row * 131 + j * (vocab // 64)) % vocab: float(j % 7 - 3)
            for j in range(ops.LOGIT_BIAS_MAX)}


def bench_kernel(B: int, rounds: int, iters: int) -> dict:
    gen = torch.Generator().manual_seed(7)
    NB = ops.LOGIT_BIAS_MAX
    logits = (torch.randn(B, VOCAB, generator=gen) * 3).to(torch.bfloat16)
    state = torch.zeros(B, VOCAB, dtype=torch.int32)
    seen = torch.rand(B, VOCAB, generator=gen) < 0.05
    state[seen] = torch.randint(1, 9, (int(seen.sum()),), generator=gen,
                                dtype=torch.int32)
    tokens = torch.randint(0, VOCAB, (B,), generator=gen)
    ids = torch.zeros(B, NB, dtype=torch.int32)
    val = torch.zeros(B, NB)
    for b in range(B):
        bias = bias_of(b, VOCAB)
        ids[b] = torch.tensor(list(bias), dtype=torch.int32)
        val[b] = torch.tensor(list(bias.values()))
    neutral = torch.tensor([[1.0, 0.0, 0.0]] * B)
    penalised = torch.tensor([[PENALTIES["repetition_penalty"],
                               PENALTIES["presence_penalty"],
                               PENALTIES["frequency_penalty"]]] * B)
    none = torch.zeros(B, dtype=torch.int32)
    full = torch.full((B,), NB, dtype=torch.int32)
    settings = {"neutral": (neutral, none, tokens),
                "penalties": (penalised, none, tokens),
                "penalties_bias64": (penalised, full, tokens),
                "penalties_no_pending": (penalised, none, None)}
    fns, equal = {}, {}
    for name, (pen, cnt, pending) in settings.items():
        host = [logits.clone(), state.clone(), pen, ids, val, cnt, pending]
        dev = [None if t is None else t.to(DEVICE) for t in host]
        ops.logit_processors(*dev)
        ops.logit_processors(*host)
        torch.cuda.synchronize()
        equal[name] = bool(
            torch.equal(dev[0].cpu().view(torch.int16),
                        host[0].view(torch.int16))
            and torch.equal(dev[1].cpu(), host[1]))
        fns[name] = (lambda dev=dev: ops.logit_processors(*dev))
    # the same penalised call over COLD_SETS copies of logits and state,
    # taken in turn: more bytes than the 256 MiB Infinity Cache holds, so
    # every call reads from HBM, as the state does in a decode step
    pen, cnt, pending = settings["penalties"]
    small = [t.to(DEVICE) for t in (pen, ids, val, cnt, pending)]
    cold = [[logits.to(DEVICE), state.to(DEVICE)] for _ in range(COLD_SETS)]
    turn = [0]

    def run_cold():
        turn[0] = (turn[0] + 1) % COLD_SETS
        ops.logit_processors(*cold[turn[0]], *small)

    fns["penalties_cold"] = run_cold
    stats = time_rounds(fns, rounds, iters, events=True)
    return {"bench": "logit_processors_kernel", "B": B, "V": VOCAB,
            "bytes": {"logits_read": B * VOCAB * 2,
                      "logits_written": B * VOCAB * 2,
                      "state_read": B * VOCAB * 4},
            "equals_cpu_branch": equal, **stats}


def bench_engine(cfg: LlamaConfig, B: int, ctx: int, rounds: int,
                 iters: int, baseline_only: bool) -> dict:
    plain = LlamaDecodeEngine(cfg, B, device=DEVICE, use_graph=True,
                              sampling="request")
    engines = {"a_request": plain}
    if not baseline_only:
        shared = dict(device=DEVICE, use_graph=True, weights=plain.weights,
                      sampling="request", logit_processors=True)
        engines["b_flag_neutral"] = LlamaDecodeEngine(cfg, B, **shared)
        engines["c_flag_penalties"] = LlamaDecodeEngine(cfg, B, **shared)
        engines["d_flag_penalties_bias64"] = LlamaDecodeEngine(cfg, B,
                                                               **shared)
        for slot in range(B):
            engines["c_flag_penalties"].set_sampling(slot, **PENALTIES)
            engines["d_flag_penalties_bias64"].set_sampling(
                slot, logit_bias=bias_of(slot, cfg.vocab_size), **PENALTIES)
    gen = torch.Generator().manual_seed(1)
    prompts = torch.randint(0, cfg.vocab_size, (B, 16), generator=gen)
    for engine in engines.values():
        engine.prefill(prompts)
        engine.capture_graph()
    result = {"bench": "decode_step_graph", "config": cfg.name,
              "layers": cfg.num_layers, "B": B, "ctx": ctx}
    if not baseline_only:
        # all rows neutral: the tokens of the engine without the flag
        plain.decode_step()
        engines["b_flag_neutral"].decode_step()
        torch.cuda.synchronize()
        result["neutral_tokens_equal_flag_off"] = torch.equal(
            plain.buf_tokens, engines["b_flag_neutral"].buf_tokens)

    def step(engine):
        def run():
            engine.cache_lens.fill_(ctx)
            engine.decode_step()
        return run

    stats = time_rounds({name: step(engine)
                         for name, engine in engines.items()},
                        rounds, iters, events=False)
    base = stats["a_request"]["median_us"]
    result.update({f"{name[:1]}_minus_a_us": round(
        stats[name]["median_us"] - base, 1) for name in list(engines)[1:]})
    result.update(stats)
    return result


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
    parser.add_argument("--baseline-only", action="store_true",
                        help="time only the engine without the flag")
    args = parser.parse_args()
    assert torch.cuda.is_available(), \
        "bench_logit_processors.py needs a GPU"
    assert ops.HAVE_HIP_OPS, "_hip_ops extension not built"

    if not args.skip_kernels:
        print(json.dumps(bench_kernel(args.batch, args.rounds, args.iters)),
              flush=True)
    if args.skip_engine:
        return
    over = {} if args.layers is None else {"num_layers": args.layers}
    cfg = LlamaConfig.llama3_8b(**over)
    print(json.dumps(bench_engine(cfg, args.batch, args.ctx, args.rounds,
                                  args.iters, args.baseline_only)),
          flush=True)


if __name__ == "__main__":
    main()
