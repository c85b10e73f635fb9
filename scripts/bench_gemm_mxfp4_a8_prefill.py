# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""Measure the W4A8 mxfp4 prefill path (prefill_gemm="mxfp4a8") on one GPU.

  python scripts/bench_gemm_mxfp4_a8_prefill.py [--skip-shapes]
                                                [--skip-engine] [--layers L]

1. Per-shape: every llama-3-8b projection at M = 128 / 640 / 2048,
   alternating in one process: the library GEMM on the dequantized bf16
   weight, ops.gemm_mxfp4 (W4A16), ops.quant_fp8_rows(swizzle=False)
   alone, ops.gemm_mxfp4_a8 alone (and both tile widths forced), and quant
   + gemm, which is what the engine runs.  Median and min-max of the
   rounds (device events around REPS calls) and, for the GEMMs, the
   achieved TFLOP/s (2 M N K over the median).
2. Engine: one prefill_packed of 640 tokens (5 prompts of 128) on three
   mxfp4w engines that share one set of weights and packs, prefill_gemm
   "library", "mxfp4" and "mxfp4a8" alternating.
Prints one JSON line per measurement.  Needs a GPU."""

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from mlrun_amd import _hip_ops, ops  # noqa: E402
from mlrun_amd.models.llama import LlamaConfig, LlamaDecodeEngine  # noqa: E402

SHAPES = {"qkv": (6144, 4096), "wo": (4096, 4096), "gate_up": (28672, 4096),
          "down": (4096, 14336), "lm_head": (128256, 4096)}
MS = (128, 640, 2048)
MODES = ("library", "mxfp4", "mxfp4a8")
ROUNDS, REPS = 9, 5


def timed(fn, n):
    start, end = torch.cuda.Event(True), torch.cuda.Event(True)
    start.record()
    for _ in range(n):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / n     # us per call


def summary(samples):
    return dict(median_us=round(statistics.median(samples), 2),
                min_us=round(min(samples), 2), max_us=round(max(samples), 2))


def alternate(calls, rounds=ROUNDS, reps=REPS):
    for fn in calls.values():
        timed(fn, 2)                             # warm-up
    samples = {mode: [] for mode in calls}
    for _ in range(rounds):
        for mode, fn in calls.items():           # alternate the modes
            samples[mode].append(timed(fn, reps))
    return samples


def bench_shape(name, n, k):
    w = (torch.randn(n, k, device="cuda") * 0.02).to(torch.bfloat16)
    w4, w_scale = ops.quantize_mxfp4_weight(w)
    w = ops.dequantize_mxfp4_weight(w4, w_scale)     # the same function
    for m in MS:
        a = torch.randn(m, k, device="cuda").to(torch.bfloat16)
        out = torch.empty(m, n, dtype=torch.bfloat16, device="cuda")
        a8, a_scale = ops.quant_fp8_rows(a, swizzle=False)

        def quant():
            ops.quant_fp8_rows(a, a8, a_scale, swizzle=False)

        def gemm():
            ops.gemm_mxfp4_a8(a8, a_scale, w4, w_scale, out=out)

        calls = {"library": lambda: torch.matmul(a, w.t(), out=out),
                 "mxfp4": lambda: ops.gemm_mxfp4(a, w4, w_scale, out=out),
                 "quant": quant, "a8": gemm,
                 "quant+a8": lambda: (quant(), gemm())}
        for bn in (64, 128):        # both widths forced, on the binding
            calls[f"a8_bn{bn}"] = lambda bn=bn: _hip_ops.gemm_mxfp4_a8_tile(
                out, a8, a_scale, w4, w_scale, bn)
        for mode, s in alternate(calls).items():
            res = summary(s)
            res.update(kind="shape", shape=name, m=m, n=n, k=k, mode=mode)
            if mode != "quant":
                res["tflops"] = round(
                    2 * m * n * k / res["median_us"] / 1e6, 1)
            print(json.dumps(res), flush=True)


def bench_engine(layers, tokens=640, prompts=5):
    cfg = LlamaConfig.llama3_8b()
    cfg.max_seq_len = 512
    if layers:
        cfg.num_layers = layers
    engines, weights = {}, None
    for mode in MODES:
        engines[mode] = LlamaDecodeEngine(
            cfg, batch_size=8, device="cuda:0", use_graph=False,
            weights=weights, weight_dtype="mxfp4w", prefill_gemm=mode)
        weights = engines[mode].weights
        engines[mode]._mx4_packs = engines[MODES[0]]._mx4_packs
    torch.cuda.synchronize()
    gen = torch.Generator().manual_seed(0)
    batch = torch.randint(0, cfg.vocab_size, (prompts, tokens // prompts),
                          generator=gen).tolist()
    calls = {mode: lambda e=engine: e.prefill_packed(batch, range(prompts))
             for mode, engine in engines.items()}
    for mode, s in alternate(calls, reps=1).items():
        res = summary(s)
        res.update(kind="prefill_packed", prefill_gemm=mode, tokens=tokens,
                   layers=cfg.num_layers)
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--skip-shapes", action="store_true")
    ap.add_argument("--skip-engine", action="store_true")
    ap.add_argument("--layers", type=int, default=0,
                    help="engine layers (0: all 32)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_gemm_mxfp4_a8_prefill.py needs a GPU")
    if not args.skip_shapes:
        for name, (n, k) in SHAPES.items():
            bench_shape(name, n, k)
    if not args.skip_engine:
        bench_engine(args.layers)


if __name__ == "__main__":
    main()
