# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""Measure prompt scoring (ops.lm_head_logprobs) on one GPU.

  python scripts/bench_lm_head_logprobs.py [--rounds R]

llama-3-8b's lm_head (V 128256, K 4096) at T = 128 / 640 / 2048, modes
alternating in one process:
  fused        ops.lm_head_logprobs (the launcher's tile width)
  fused_bn64 / fused_bn128     the width forced
  fused_bn64_nfast / fused_bn128_nfast   column tiles fastest in the grid
               (order 1 of the binding; the default is M tiles fastest)
  gemm_bf16    ops.gemm_bf16 + torch.log_softmax + gather
  matmul       torch.matmul + torch.log_softmax + gather
Median and min-max of the rounds (device events around REPS calls), and
for fused and matmul torch.cuda.max_memory_allocated() above the operands.
Prints one JSON line per measurement.  Needs a GPU."""

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from mlrun_amd import _hip_ops, ops  # noqa: E402

V, K = 128256, 4096
TS = (128, 640, 2048)
REPS = 3


def timed(fn, n):
    start, end = torch.cuda.Event(True), torch.cuda.Event(True)
    start.record()
    for _ in range(n):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / n     # us per call


def peak_above(fn):
    """Peak allocated bytes of one call above what is allocated now."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def bench(t, w, rounds):
    h = torch.randn(t, K, device="cuda").to(torch.bfloat16)
    targets = torch.randint(0, V, (t,), device="cuda", dtype=torch.int32)
    idx = targets.long()[:, None]
    out = torch.empty(3, t, dtype=torch.float32, device="cuda")
    ws = torch.empty(ops.lm_head_logprobs_ws_numel(t, V),
                     dtype=torch.float32, device="cuda")

    def unfused(gemm):
        return torch.log_softmax(gemm(h, w).float(), -1).gather(1, idx)

    calls = {"fused": lambda: ops.lm_head_logprobs(h, w, targets, out=out,
                                                   workspace=ws)}
    for bn in (64, 128):
        for order, tag in ((0, ""), (1, "_nfast")):
            calls[f"fused_bn{bn}{tag}"] = lambda bn=bn, order=order: \
                _hip_ops.lm_head_logprobs(out, ws, h, w, targets, bn, order)
    calls["gemm_bf16"] = lambda: unfused(ops.gemm_bf16)
    calls["matmul"] = lambda: unfused(lambda a, b: torch.matmul(a, b.t()))
    for fn in calls.values():
        timed(fn, 1)                             # warm-up
    samples = {mode: [] for mode in calls}
    for _ in range(rounds):
        for mode, fn in calls.items():           # alternate the modes
            samples[mode].append(timed(fn, REPS))
    for mode, s in samples.items():
        res = dict(t=t, v=V, k=K, mode=mode,
                   median_us=round(statistics.median(s), 1),
                   min_us=round(min(s), 1), max_us=round(max(s), 1))
        if mode in ("fused", "matmul"):
            # fused: out and workspace are its own memory, count them
            extra = out.numel() * 4 + ws.numel() * 4 if mode == "fused" else 0
            res["peak_mb_above_operands"] = round(
                (peak_above(calls[mode]) + extra) / 2 ** 20, 1)
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_lm_head_logprobs.py needs a GPU")
    w = (torch.randn(V, K, device="cuda") * 0.02).to(torch.bfloat16)
    for t in TS:
        bench(t, w, args.rounds)


if __name__ == "__main__":
    main()
