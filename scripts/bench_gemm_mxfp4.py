# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""Measure the mxfp4w decode mode against bf16 and fp8w on one GPU.

  python scripts/bench_gemm_mxfp4.py [--skip-step] [--layers L]

1. Per-shape: every llama-3-8b projection at batch 32, the three weight
   modes alternating in one process.  Each mode rotates over enough
   weight copies that no copy is still in the 256 MiB Infinity Cache
   when its turn comes again.  Median and min-max of the rounds (device
   events around REPS calls), and the weight bytes per second.
2. In-step: three engines on one set of weights under hipGraph replay
   at context 160; median and min-max of 15 rounds of 20 replays.
The per-shape part also times fp8w's stand-alone activation quantization;
--sweep times mxfp4w at other ksplits.  MLRUN_GEMM_PLAN overrides the
plan for an in-step comparison of two splits.
Prints one JSON line per measurement.  Needs a GPU."""

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from mlrun_amd import ops  # noqa: E402
from mlrun_amd.models.llama import LlamaConfig, LlamaDecodeEngine  # noqa: E402

B = 32
SHAPES = {"qkv": (6144, 4096), "wo": (4096, 4096), "gate_up": (28672, 4096),
          "down": (4096, 14336), "lm_head": (128256, 4096)}
ROTATE_BYTES = 768 << 20     # 3x the Infinity Cache between two visits
ROUNDS, REPS = 15, 20


def timed(fn, n):
    start, end = torch.cuda.Event(True), torch.cuda.Event(True)
    start.record()
    for i in range(n):
        fn(i)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / n     # us per call


def summary(samples):
    return dict(median_us=round(statistics.median(samples), 2),
                min_us=round(min(samples), 2), max_us=round(max(samples), 2))


def bench_shape(name, n, k):
    ksplit, variant = ops.pick_gemm_plan(B, n, k)
    ksplits = {"bf16": ksplit, "fp8w": ksplit,
               "mxfp4w": ops.pick_mxfp4_ksplit(B, n, k)}
    a = torch.randn(B, k, device="cuda").to(torch.bfloat16)
    out = torch.empty(B, n, dtype=torch.bfloat16, device="cuda")
    c32 = torch.empty(max(ksplit, 4) * B * n, device="cuda")
    w = (torch.randn(n, k, device="cuda") * 0.02).to(torch.bfloat16)
    a8, a_scale = ops.quant_fp8_rows(a)
    packs = {"bf16": (w,), "fp8w": ops.quantize_fp8_weight(w),
             "mxfp4w": ops.quantize_mxfp4_weight(w)}
    calls, nbytes = {}, {}
    for mode, pack in packs.items():
        nbytes[mode] = sum(t.numel() * t.element_size() for t in pack)
        copies = [tuple(t.clone() for t in pack)
                  for _ in range(ROTATE_BYTES // nbytes[mode] + 2)]
        if mode == "bf16":
            calls[mode] = lambda i, c=copies: ops.skinny_gemm(
                a, c[i % len(c)][0], out=out, c_f32=c32, ksplit=ksplit,
                variant=variant)
        elif mode == "fp8w":
            calls[mode] = lambda i, c=copies: ops.skinny_gemm_fp8(
                a8, a_scale, *c[i % len(c)], out=out, c_f32=c32,
                ksplit=ksplit)
        else:
            calls[mode] = lambda i, c=copies: ops.skinny_gemm_mxfp4(
                a, *c[i % len(c)], out=out, c_f32=c32,
                ksplit=ksplits["mxfp4w"])
    samples = {mode: [] for mode in calls}
    for mode, fn in calls.items():
        timed(fn, REPS)                          # warm-up
    for _ in range(ROUNDS):
        for mode, fn in calls.items():           # alternate the modes
            samples[mode].append(timed(fn, REPS))
    for mode, s in samples.items():
        res = summary(s)
        res.update(kind="shape", shape=name, n=n, k=k, batch=B, mode=mode,
                   ksplit=ksplits[mode], weight_bytes=nbytes[mode],
                   weight_tb_s=round(nbytes[mode] / res["median_us"] / 1e6,
                                     3))
        print(json.dumps(res), flush=True)


def bench_sweep(name, n, k):
    """mxfp4w alone at other ksplits than the plan table's."""
    a = torch.randn(B, k, device="cuda").to(torch.bfloat16)
    out = torch.empty(B, n, dtype=torch.bfloat16, device="cuda")
    c32 = torch.empty(8 * B * n, device="cuda")
    pack = ops.quantize_mxfp4_weight(
        (torch.randn(n, k, device="cuda") * 0.02).to(torch.bfloat16))
    nbytes = sum(t.numel() for t in pack)
    copies = [tuple(t.clone() for t in pack)
              for _ in range(ROTATE_BYTES // nbytes + 2)]
    for ksplit in (1, 2, 4, 8):
        def call(i):
            ops.skinny_gemm_mxfp4(a, *copies[i % len(copies)], out=out,
                                  c_f32=c32, ksplit=ksplit)
        timed(call, REPS)
        res = summary([timed(call, REPS) for _ in range(ROUNDS)])
        res.update(kind="sweep", shape=name, mode="mxfp4w", ksplit=ksplit)
        print(json.dumps(res), flush=True)


def bench_quant():
    """The activation quantization that fp8w launches in front of wo and
    down (qkv, gate_up and lm_head take the RMSNorm sidecar)."""
    for k in (4096, 14336):
        a = torch.randn(B, k, device="cuda").to(torch.bfloat16)
        a8, a_scale = ops.quant_fp8_rows(a)
        timed(lambda i: ops.quant_fp8_rows(a, a8, a_scale), REPS)
        res = summary([timed(lambda i: ops.quant_fp8_rows(a, a8, a_scale),
                             REPS) for _ in range(ROUNDS)])
        res.update(kind="quant_fp8_rows", batch=B, k=k)
        print(json.dumps(res), flush=True)


def bench_step(layers, context=160):
    cfg = LlamaConfig.llama3_8b()
    cfg.max_seq_len = 512
    if layers:
        cfg.num_layers = layers
    engines, weights = {}, None
    for mode in ("bf16", "fp8w", "mxfp4w"):
        engines[mode] = LlamaDecodeEngine(cfg, batch_size=B, device="cuda:0",
                                          use_graph=True, weights=weights,
                                          weight_dtype=mode)
        weights = engines[mode].weights
    prompt = torch.randint(0, cfg.vocab_size, (B, context),
                           generator=torch.Generator().manual_seed(0))
    for engine in engines.values():
        engine.generate(prompt, max_new_tokens=4)     # prefill + capture
    samples = {mode: [] for mode in engines}
    for _ in range(ROUNDS):
        for mode, engine in engines.items():
            engine.cache_lens.fill_(context)
            samples[mode].append(
                timed(lambda i, e=engine: e.decode_step(), REPS))
    for mode, s in samples.items():
        res = summary(s)
        res.update(kind="step", mode=mode, batch=B, context=context,
                   layers=cfg.num_layers)
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-shapes", action="store_true")
    ap.add_argument("--sweep", action="store_true",
                    help="also time mxfp4w at ksplit 1, 2, 4, 8 per shape")
    ap.add_argument("--layers", type=int, default=0,
                    help="engine layers for the in-step timing (0: all 32)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_gemm_mxfp4.py needs a GPU")
    if not args.skip_shapes:
        for name, (n, k) in SHAPES.items():
            bench_shape(name, n, k)
        bench_quant()
    if args.sweep:
        for name, (n, k) in SHAPES.items():
            bench_sweep(name, n, k)
    if not args.skip_step:
        bench_step(args.layers)


if __name__ == "__main__":
    main()
