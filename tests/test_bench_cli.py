# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""bench.py command-line contract: result line, --dump-outputs, --full
(CPU tiny config — the same code path the GPU run takes)."""

import json
import os
import subprocess
import sys

import numpy as np

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(*extra):
    proc = subprocess.run(
        [sys.executable, os.path.join(REPO_ROOT, "bench.py"), "--gpus", "1",
         "--steps", "3", "--warmup", "1", "--model", "tiny", "--batch", "2",
         "--prompt-len", "8", "--gen-tokens", "8", *extra],
        cwd=REPO_ROOT, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-2000:]
    return json.loads(proc.stdout.strip().splitlines()[-1])


def test_dump_outputs_repeatable_and_full(tmp_path):
    first = _run_bench("--dump-outputs", str(tmp_path / "a"))
    second = _run_bench("--full", "--dump-outputs", str(tmp_path / "b"))
    for result in (first, second):
        for key in ("metric", "value", "unit", "higher_is_better", "dtype",
                    "ms_per_step"):
            assert key in result, key
        assert result["steps"] == 3
        assert result["ms_per_step"] > 0
        # value and ms_per_step describe the same timed steps
        per_step = result["config"]["global_batch"] / result["value"] * 1e3
        assert abs(per_step - result["ms_per_step"]) < \
            0.01 * result["ms_per_step"]
    a = np.load(tmp_path / "a" / "outputs.npy")
    b = np.load(tmp_path / "b" / "outputs.npy")
    assert a.dtype == np.float32
    assert a.shape == (first["config"]["global_batch"],
                       first["config"]["gen_tokens"])
    assert np.array_equal(a, b)
