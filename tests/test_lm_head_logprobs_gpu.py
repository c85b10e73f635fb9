# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""lm_head_logprobs_kernel: its logits are gemm_bf16_tile_kernel's bit for
bit, its log-sum-exp against float64, its memory accesses, and
LlamaDecodeEngine.score_packed on it.

The lse bound, from the code (u = 2^-24; expf and logf are within 1 ulp =
2 u; NI = BN / 32 accumulators per lane and row, P = ceil(V / BN) partials
per row).  Relative error of l = sum exp(z - M), every term positive:
  wave:  z - m rounded (u, weighted by |x| e^-|x| < 1), expf (2 u), a chain
         of 4 NI - 1 register additions and 2 cross-lane ones:
         (4 NI + 4) u
  workgroup: m - M rounded, expf, the product, one addition: 5 u
  fold:  m_p - M rounded, expf, the product (4 u), ceil(P / 64) - 1
         additions in the lane and 6 in the butterfly
so n = 4 NI + 18 + ceil(P / 64) roundings, gamma = n u / (1 - n u); the
maxima are exact.  lse = fl(M + logf(l)): |d log l| <= gamma, logf adds
2 u |log l|, the last addition u |lse|."""

import functools
import math

import pytest
import torch

from mlrun_amd import ops

from decode_refs import EPS32, MEASURED, check, f64
from lm_head_refs import check_score_packed

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs MI355X")]


@functools.lru_cache(maxsize=None)
def case(t, v, k):
    """Seeded N(0,1) bf16 operands; targets walk over column 0, V - 1, a
    mid column, -1 and V (the first clamped column)."""
    g = torch.Generator().manual_seed(10 * k + t + v)
    h = torch.randn(t, k, generator=g).to(torch.bfloat16)
    w = torch.randn(v, k, generator=g).to(torch.bfloat16)
    targets = torch.tensor([0, v - 1, v // 2, -1, v],
                           dtype=torch.int32).repeat(t // 5 + 1)[:t]
    return h, w, targets


def score(h, w, targets, bn):
    """(logprob, lse, z_tgt) of the op, and the sibling GEMM's logits of the
    same rows as float64, from a call of at least 65 rows at the same bn."""
    t, width = h.shape[0], bn or 64  # bn 0 picks 64 at sizes this small
    out = torch.empty(3, t, dtype=torch.float32, device="cuda")
    logprob, lse = ops.lm_head_logprobs(h, w, targets, out=out, bn=bn)
    rows = torch.zeros(max(t, 65), h.shape[1], dtype=h.dtype, device="cuda")
    rows[:t] = h
    z = torch.empty(rows.shape[0], w.shape[0], dtype=h.dtype, device="cuda")
    ops._require_hip().gemm_bf16_tile(z, rows, w, width)
    return logprob, lse, out[2], z[:t]


def check_scores(h, w, targets, bn, what):
    v, width = w.shape[0], bn or 64
    logprob, lse, z_tgt, z = score(h.cuda(), w.cuda(), targets.cuda(), bn)
    inside = ((targets >= 0) & (targets < v)).cuda()
    want = z.gather(1, targets.cuda().long().clamp(0, v - 1)[:, None])[:, 0]
    assert torch.equal(z_tgt[inside], want[inside].float()), what
    assert (z_tgt[~inside] == 0).all(), what
    assert torch.equal(logprob[~inside], -lse[~inside]), what
    assert torch.equal(logprob, z_tgt - lse), what
    z = f64(z)
    ref = torch.logsumexp(z, -1)
    n = 4 * (width // 32) + 18 + math.ceil(math.ceil(v / width) / 64)
    gamma = n * EPS32 / (1 - n * EPS32)
    bound = gamma + 2 * EPS32 * (ref - z.amax(-1)) + EPS32 * ref.abs()
    check(lse, ref, bound, f"lse {what} bn{bn}", kernel="lm_head_logprobs")


# T: below one wave's rows, one or two M tiles, full and ragged; V: one
# clamped tile, an exact one, several with a ragged last; K: the 32-k tail
# alone, a stage plus the tail, a long loop.
@pytest.mark.parametrize("bn", [0, 128])
@pytest.mark.parametrize("k", [32, 96, 1120])
@pytest.mark.parametrize("v", [80, 128, 272])
@pytest.mark.parametrize("t", [1, 65, 129, 200])
def test_logits_are_the_gemms_and_lse_against_float64(t, v, k, bn):
    check_scores(*case(t, v, k), bn, f"t{t} v{v} k{k}")


@pytest.mark.parametrize("bn", [0, 128])
def test_tile_maxima_far_apart(bn):
    """h scaled by 8: logits of std ~80, so the partials of a row have
    maxima tens apart and the fold's rescale decides the result."""
    h, w, targets = case(129, 272, 96)
    check_scores(h * 8, w, targets, bn, "h * 8")


@pytest.mark.parametrize("bn", [0, 128])
@pytest.mark.parametrize("v", [80, 272])
def test_row_maximum_in_the_last_column_of_a_ragged_tile(v, bn):
    """Column 0 of h is 6 and w[V - 1, 0] is 30: logit V - 1 is about 180
    above the others (std ~10) in every row.  The clamped columns >= V
    repeat it; unmasked, each would add log 2 or more to lse."""
    h, w, targets = (x.clone() for x in case(65, v, 96))
    h[:, 0], w[v - 1, 0] = 6.0, 30.0
    check_scores(h, w, targets, bn, f"max in column {v - 1}")


@pytest.mark.parametrize("bn", [64, 128])
def test_memory_past_the_operands_is_never_touched(bn):
    """Each operand ends its buffer and bf16 NaN follows; the outputs and
    the workspace sit between sentinels, which stay."""
    t, v, k = 129, 80, 96
    h, w, targets = case(t, v, k)

    def guarded(x):
        buf = torch.full((2 * x.numel(),), float("nan"), dtype=x.dtype,
                         device="cuda")
        buf[:x.numel()] = x.flatten().cuda()
        return buf[:x.numel()].view(x.shape)

    need = ops.lm_head_logprobs_ws_numel(t, v)
    frame = torch.full((5, t), 77.0, device="cuda")
    ws_frame = torch.full((need + 16,), 77.0, device="cuda")
    logprob, lse = ops.lm_head_logprobs(
        guarded(h), guarded(w), targets.cuda(), out=frame[1:4],
        workspace=ws_frame[8:8 + need], bn=bn)
    assert (frame[0] == 77.0).all() and (frame[4] == 77.0).all()
    assert (ws_frame[:8] == 77.0).all() and (ws_frame[8 + need:] == 77.0).all()
    clean = score(h.cuda(), w.cuda(), targets.cuda(), bn)
    assert torch.equal(lse, clean[1]) and torch.equal(logprob, clean[0])
    assert torch.isfinite(lse).all()


def test_score_packed_against_prefix_prefills():
    check_score_packed("cuda:0")
    print("largest lse err/bound", MEASURED.get("lm_head_logprobs"))
