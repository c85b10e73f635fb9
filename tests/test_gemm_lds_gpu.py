# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""LDS-DMA ring decode GEMM (variant 4) against the register-ring kernel
(variant 1): the two share decomposition, k order and MFMA operand map,
so every result must be bit-identical.  Operands are interior slices of
NaN-fenced buffers: a row fetched from outside a tensor poisons the
output.

The ring is chosen by MLRUN_GEMM_LDS_RING, which the extension reads
once per process, so `test_all_rings` re-runs this file's cases in one
child process per ring; the cases themselves run under the default."""

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
RINGS = ("64x2", "64x3", "128x2")

# (M, N, K, ksplit): the smallest shapes at which each mechanism of the
# ring kernel can go wrong
CASES = [
    (32, 32, 128, 1),    # 32 k per wave: no full stage, tail only
    (32, 32, 256, 1),    # exactly one 64-k stage
    (32, 32, 512, 1),    # exactly DEPTH=2 stages of 64 / one of 128
    (32, 64, 1792, 1),   # 7 stages of 64: ring wraps, then drains;
                         #   128x2: 3 stages + a 64-k tail
    (32, 32, 160, 1),    # waves get 64/64/32/0 k: wave 3 is empty
    (17, 48, 1056, 2),   # clamped A rows, partial n-tile, uneven split-K
    (32, 96, 2048, 4),   # split-K slabs
]
FALLBACK = [(16, 64, 512, 1), (48, 64, 512, 1)]


def _fenced(rows, k, seed):
    """[rows, k] bf16 slice in the middle of a buffer whose other rows
    are NaN."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((rows + 2, k), float("nan"), dtype=torch.bfloat16)
    buf[1:rows + 1] = (torch.randn(rows, k, generator=g) * 0.5).to(
        torch.bfloat16)
    buf = buf.cuda()
    return buf[1:rows + 1]


def _operands(m, n, k):
    a = _fenced(m, k, seed=1000 + m + k)
    w = _fenced(n, k, seed=2000 + n + k)
    assert a.is_contiguous() and w.is_contiguous()
    return a, w


def _check(m, n, k, ksplit):
    from mlrun_amd import ops

    a, w = _operands(m, n, k)
    ref = ops.skinny_gemm(a, w, ksplit=ksplit, variant=1)
    got = ops.skinny_gemm(a, w, ksplit=ksplit, variant=4)
    torch.cuda.synchronize()
    assert torch.equal(ref, got), \
        f"variant 4 != variant 1 at {(m, n, k, ksplit)}: " \
        f"{(ref.float() - got.float()).abs().max().item()}"
    exact = a.float() @ w.float().t()
    err = (exact - got.float()).abs().max().item()
    assert err < 0.02 * math.sqrt(k), f"max err {err} at {(m, n, k)}"


@requires_gpu
@pytest.mark.parametrize("m,n,k,ksplit", CASES)
def test_bit_identical(m, n, k, ksplit):
    _check(m, n, k, ksplit)


@requires_gpu
@pytest.mark.parametrize("m,n,k,ksplit", FALLBACK)
def test_fallback_is_variant1(m, n, k, ksplit):
    """M <= 16 and M > 32 run what variant 1 runs."""
    _check(m, n, k, ksplit)


@requires_gpu
def test_slabs_bit_identical():
    import mlrun_amd._hip_ops as ext

    m, n, k, ksplit = 32, 96, 2048, 4
    a, w = _operands(m, n, k)
    ref = torch.full((ksplit * m * n,), float("nan"), dtype=torch.float32,
                     device="cuda")
    got = ref.clone()
    ext.skinny_gemm_slabs(ref, a, w, ksplit, 1)
    ext.skinny_gemm_slabs(got, a, w, ksplit, 4)
    torch.cuda.synchronize()
    assert not torch.isnan(got).any()
    assert torch.equal(ref, got)


@requires_gpu
def test_graph_capture():
    from mlrun_amd import ops

    m, n, k = 32, 64, 1792
    a, w = _operands(m, n, k)
    a2 = _fenced(m, k, seed=77)
    a1 = a.clone()
    out = torch.empty(m, n, dtype=torch.bfloat16, device="cuda")
    eager1 = ops.skinny_gemm(a1, w, ksplit=1, variant=4).clone()
    eager2 = ops.skinny_gemm(a2, w, ksplit=1, variant=4).clone()
    torch.cuda.synchronize()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.skinny_gemm(a, w, out=out, ksplit=1, variant=4)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.skinny_gemm(a, w, out=out, ksplit=1, variant=4)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager1)
    a.copy_(a2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager2)


def _run_all_cases():
    for case in CASES + FALLBACK:
        _check(*case)
    test_slabs_bit_identical()
    test_graph_capture()


@requires_gpu
@pytest.mark.parametrize("ring", RINGS)
def test_all_rings(ring):
    """Every case above with the ring fixed by the environment knob."""
    env = dict(os.environ, MLRUN_GEMM_LDS_RING=ring)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    proc = subprocess.run([sys.executable, os.path.abspath(__file__)],
                          cwd=REPO, env=env, capture_output=True, text=True,
                          timeout=300)
    assert proc.returncode == 0 and "ring ok" in proc.stdout, \
        f"ring {ring}:\n{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}"


if __name__ == "__main__":
    _run_all_cases()
    print("ring ok", os.environ.get("MLRUN_GEMM_LDS_RING"))
