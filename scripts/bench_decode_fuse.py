# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""Time the captured decode step with the bit-exact fusions off and on.

  python scripts/bench_decode_fuse.py [--layers L]

llama-3-8b, batch 32, context 160, hipGraph replay: four engines on one
set of weights, captured with MLRUN_DECODE_FUSE at none / norm / swiglu /
norm,swiglu, alternate in one process; median and min-max of 15 rounds
of 20 replays each.  Before timing, every engine's logits and tokens
after the same steps must equal the `none` engine's bit for bit.
Prints one JSON line per setting.  Needs a GPU."""

import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from mlrun_amd.models.llama import LlamaConfig, LlamaDecodeEngine  # noqa: E402

B, CONTEXT = 32, 160
ROUNDS, REPS = 15, 20
SETTINGS = ("none", "norm", "swiglu", "norm,swiglu")


def timed(fn, n):
    start, end = torch.cuda.Event(True), torch.cuda.Event(True)
    start.record()
    for _ in range(n):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / n     # us per call


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--layers", type=int, default=0,
                    help="engine layers (0: all 32)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_decode_fuse.py needs a GPU")
    cfg = LlamaConfig.llama3_8b()
    cfg.max_seq_len = 512
    if args.layers:
        cfg.num_layers = args.layers
    prompt = torch.randint(0, cfg.vocab_size, (B, CONTEXT),
                           generator=torch.Generator().manual_seed(0))
    engines, weights = {}, None
    for setting in SETTINGS:
        # the knob is read when the step is captured
        os.environ["MLRUN_DECODE_FUSE"] = setting
        engine = LlamaDecodeEngine(cfg, batch_size=B, device="cuda:0",
                                   use_graph=True, weights=weights)
        weights = engine.weights
        engine.generate(prompt, max_new_tokens=4)     # prefill + capture
        engines[setting] = engine
    torch.cuda.synchronize()
    ref = engines["none"]
    for setting, engine in engines.items():
        if not (torch.equal(engine.buf_logits, ref.buf_logits) and
                torch.equal(engine.buf_tokens, ref.buf_tokens)):
            sys.exit(f"MLRUN_DECODE_FUSE={setting} changed the outputs")
    samples = {setting: [] for setting in engines}
    for _ in range(ROUNDS):
        for setting, engine in engines.items():      # alternate
            engine.cache_lens.fill_(CONTEXT)
            samples[setting].append(timed(engine.decode_step, REPS))
    for setting, s in samples.items():
        print(json.dumps(dict(
            kind="step", fuse=setting, batch=B, context=CONTEXT,
            layers=cfg.num_layers, median_us=round(statistics.median(s), 2),
            min_us=round(min(s), 2), max_us=round(max(s), 2))), flush=True)


if __name__ == "__main__":
    main()
