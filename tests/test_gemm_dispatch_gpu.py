# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""The dispatch table of the bf16 skinny GEMM, cell by cell: every
(variant, M class, ksplit) cell of ``ops.skinny_gemm`` must launch a
kernel that computes the product, and the variants that share a
decomposition must agree bit for bit.  Operands are interior slices of
NaN-fenced buffers and the output starts as NaN, so a cell that launches
nothing, a wrong grid or a row fetched from outside a tensor shows.

N = 80 is a partial tile for the 32- and 128-wide kernels and exactly
five tiles for variant 3's 16-wide ones; M = 17 and 33 are the first rows
of the MT=2 and MT=4 classes.  MLRUN_GEMM_PIPE and MLRUN_GEMM_UNR2 pick
the M in (16, 32] kernel of variants 1 and 2 and are read once per
process, so `test_mt2_knobs` runs those cells in one child process per
setting."""

import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K = 80, 512
BOUND = 0.02 * math.sqrt(K)  # the project's bound for a bf16 GEMM
VARIANTS = (0, 1, 2, 3, 4)
MS = (16, 17, 33)
KSPLITS = (1, 2)
# the M in (16, 32] kernels of variant 1: burst-unrolled at depth 4 and
# 8, and the pipelined ring at depth 3 and 6 (the default is 4)
KNOBS = (
    {"MLRUN_GEMM_PIPE": "0"},
    {"MLRUN_GEMM_PIPE": "0", "MLRUN_GEMM_UNR2": "8"},
    {"MLRUN_GEMM_PIPE": "3"},
    {"MLRUN_GEMM_PIPE": "6"},
)


def _fenced(rows, k, seed):
    """[rows, k] bf16 slice in the middle of a buffer whose other rows
    are NaN."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((rows + 2, k), float("nan"), dtype=torch.bfloat16)
    buf[1:rows + 1] = (torch.randn(rows, k, generator=g) * 0.5).to(
        torch.bfloat16)
    buf = buf.cuda()
    return buf[1:rows + 1]


_OPERANDS = {}


def _operands(m):
    """(a, w, exact fp32 product) for M = m, built once."""
    if m not in _OPERANDS:
        a = _fenced(m, K, seed=3000 + m)
        w = _fenced(N, K, seed=4000)
        assert a.is_contiguous() and w.is_contiguous()
        _OPERANDS[m] = (a, w, a.float() @ w.float().t())
    return _OPERANDS[m]


def _run(m, ksplit, variant):
    """One cell: the output, checked for NaN and against fp32."""
    from mlrun_amd import ops

    a, w, exact = _operands(m)
    out = torch.full((m, N), float("nan"), dtype=torch.bfloat16,
                     device="cuda")
    got = ops.skinny_gemm(a, w, out=out, ksplit=ksplit, variant=variant)
    torch.cuda.synchronize()
    cell = f"variant {variant}, M {m}, ksplit {ksplit}"
    assert not torch.isnan(got).any(), f"NaN left in the output: {cell}"
    err = (exact - got.float()).abs().max().item()
    assert err < BOUND, f"max err {err} >= {BOUND}: {cell}"
    return got


@requires_gpu
@pytest.mark.parametrize("ksplit", KSPLITS)
@pytest.mark.parametrize("m", MS)
def test_dispatch_cells(m, ksplit):
    """All five variants of one (M, ksplit): each is right, and
    variants 2 and 4 equal variant 1 bit for bit."""
    got = {variant: _run(m, ksplit, variant) for variant in VARIANTS}
    for variant in (2, 4):
        assert torch.equal(got[variant], got[1]), \
            f"variant {variant} != variant 1 at M {m}, ksplit {ksplit}: " \
            f"{(got[variant].float() - got[1].float()).abs().max().item()}"


def _run_mt2_cells():
    for ksplit in KSPLITS:
        _run(17, ksplit, 1)


@requires_gpu
@pytest.mark.parametrize("knobs", KNOBS,
                         ids=lambda k: ",".join(f"{a[11:]}={b}"
                                                for a, b in k.items()))
def test_mt2_knobs(knobs):
    """Variant 1's M = 17 cells with the kernel fixed by the knobs."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("MLRUN_GEMM_PIPE", "MLRUN_GEMM_UNR2")}
    env.update(knobs)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    proc = subprocess.run([sys.executable, os.path.abspath(__file__)],
                          cwd=REPO, env=env, capture_output=True, text=True,
                          timeout=300)
    assert proc.returncode == 0 and "cells ok" in proc.stdout, \
        f"{knobs}:\n{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}"


if __name__ == "__main__":
    _run_mt2_cells()
    print("cells ok", os.environ.get("MLRUN_GEMM_PIPE"),
          os.environ.get("MLRUN_GEMM_UNR2"))
