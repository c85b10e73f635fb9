# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""GPU numerics of the segmented multi-LoRA prefill kernels
(lora_sgmv_shrink_kernel / lora_sgmv_expand_kernel) against float64, on
the five-segment layout of test_lora_sgmv.py, and of
``lora_prefill="sgmv"`` in LlamaDecodeEngine.

Largest err / bound measured on an MI355X: shrink 0.0127 (K = 32; 0.0022
at K = 160, below 0.0002 from K = 1056 on), expand 0.9898 (the final
bf16 rounding next to a power of two; 0.9868 / 0.9898 / 0.9873 / 0.9756
for R = 8 / 16 / 32 / 64).  The same expand inputs with t rounded to bf16
once miss the bound by 64 x (R = 64) to 164 x (R = 8).  Engine: "sgmv"
against "library" 0.0117, against merged weights 0.0195, bound 0.0469."""

import pytest
import torch

from decode_refs import R1
from test_lora_sgmv import (COUNTS, IDS, NA, RANKS, T, TILES,
                            check_engine_sgmv, covered, int_case)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

# one MFMA step (seven idle waves), fewer steps than waves, uneven shares
# with an unrolled body and a tail; 4128 = 129 steps: every wave runs the
# four-step body
KS = (32, 160, 1056, 4128)
# half a fragment, across a wave's 64-column edge, across the
# workgroup's 256-column edge
NS = (8, 72, 264)
ROWS = covered()
BASE_ROWS = [r for r in range(T) if r not in ROWS]


def _tiles():
    from mlrun_amd import ops

    return ops.lora_sgmv_tiles(COUNTS, IDS, "cuda")


def _shrink(x, A, tiles=None, fill=0.0):
    from mlrun_amd import ops

    t = torch.full((x.shape[0], A.shape[1]), fill, device="cuda")
    ops.lora_sgmv_shrink(x.cuda(), A.cuda(),
                         _tiles() if tiles is None else tiles, out=t)
    return t.cpu()


def _expand(y, t, Bm, tiles=None):
    from mlrun_amd import ops

    return ops.lora_sgmv_expand(y.cuda(), t.cuda(), Bm.cuda(),
                                _tiles() if tiles is None else tiles).cpu()


def _rand_case(R, K, N, seed):
    gen = torch.Generator().manual_seed(seed)

    def bf16(*shape):
        return torch.randn(*shape, generator=gen).to(torch.bfloat16)

    return dict(x=bf16(T, K), A=bf16(NA, R, K), Bm=bf16(NA, N, R),
                y0=bf16(T, N), t=torch.randn(T, R, generator=gen))


@requires_gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("R", RANKS)
def test_shrink_vs_float64(R, K):
    """|t - ref| <= 2 K 2^-24 (|x| @ |A_a|^T), the worst case of an f32
    sum in any order; rows outside every tile keep the fill value."""
    case = _rand_case(R, K, 8, 100 * R + K)
    got = _shrink(case["x"], case["A"], fill=7.5)
    assert (got[BASE_ROWS] == 7.5).all()
    worst = 0.0
    for r0, n, a in TILES:
        x, A = case["x"][r0:r0 + n].double(), case["A"][a].double()
        bound = 2 * K * 2.0 ** -24 * (x.abs() @ A.abs().t())
        err = (got[r0:r0 + n].double() - x @ A.t()).abs()
        worst = max(worst, (err / bound).max().item())
    print(f"shrink R={R} K={K}: err/bound {worst:.4f}")
    assert worst <= 1.0


@requires_gpu
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("R", RANKS)
def test_expand_vs_float64(R, N):
    """|out - ref| <= R1 |ref| + (2^-18 + (2 R + 2) 2^-24) (|y| + |t| @
    |Bm_a|^T): one bf16 rounding, the hi/lo residual of t, and 2 R + 1 f32
    additions.  randn inputs: many outputs cancel far below their terms,
    where a t rounded to bf16 once (2^-9 per term) breaks the bound."""
    case = _rand_case(R, 32, N, 100 * R + N)
    got = _expand(case["y0"], case["t"], case["Bm"])
    assert torch.equal(got[BASE_ROWS], case["y0"][BASE_ROWS])
    worst = 0.0
    for r0, n, a in TILES:
        y, t = case["y0"][r0:r0 + n].double(), case["t"][r0:r0 + n].double()
        Bm = case["Bm"][a].double()
        ref = y + t @ Bm.t()
        bound = R1 * ref.abs() + (2.0 ** -18 + (2 * R + 2) * 2.0 ** -24) * (
            y.abs() + t.abs() @ Bm.abs().t())
        err = (got[r0:r0 + n].double() - ref).abs()
        worst = max(worst, (err / bound).max().item())
    print(f"expand R={R} N={N}: err/bound {worst:.4f}")
    assert worst <= 1.0


@requires_gpu
@pytest.mark.parametrize("R", RANKS)
def test_integer_exact(R):
    for K, N in ((32, 8), (160, 72), (1056, 264)):
        case = int_case(R, K, N, seed=R + K)
        t = _shrink(case["x"], case["A"])
        assert torch.equal(t[ROWS], case["t_exp"][ROWS]), (K, N)
        y = _expand(case["y0"], case["t_exp"], case["Bm"])
        assert torch.equal(y, case["y_exp"]), (K, N)


@requires_gpu
@pytest.mark.parametrize("R", RANKS)
def test_poison_stays_out(R):
    """NaN in the adapter slot that nothing names and in the x and t
    rows that no tile covers: never read, never written."""
    case = _rand_case(R, 160, 264, R)
    t_ref = _shrink(case["x"], case["A"])
    y_ref = _expand(case["y0"], case["t"], case["Bm"])
    x, t, A, Bm = (case[k].clone() for k in ("x", "t", "A", "Bm"))
    x[BASE_ROWS] = t[BASE_ROWS] = A[3] = Bm[3] = float("nan")
    t_got, y_got = _shrink(x, A), _expand(case["y0"], t, Bm)
    assert torch.isfinite(t_got).all() and torch.equal(t_got, t_ref)
    assert torch.isfinite(y_got.float()).all() and torch.equal(y_got, y_ref)
    assert torch.equal(y_got[BASE_ROWS], case["y0"][BASE_ROWS])


@requires_gpu
@pytest.mark.parametrize("R", RANKS)
def test_row_independence(R):
    """The rows of a prompt alone give the bits they give in the
    five-segment call."""
    from mlrun_amd import ops

    case = _rand_case(R, 1056, 264, 7 * R)
    t_all = _shrink(case["x"], case["A"])
    y_all = _expand(case["y0"], case["t"], case["Bm"])
    for r0, n, a in ((34, 5, 2), (39, 33, 1), (1, 16, 0)):
        alone = ops.lora_sgmv_tiles([n], [a], "cuda")
        rows = slice(r0, r0 + n)
        t = _shrink(case["x"][rows], case["A"], alone)
        y = _expand(case["y0"][rows], case["t"][rows], case["Bm"], alone)
        assert torch.equal(t, t_all[rows]) and torch.equal(y, y_all[rows])


@requires_gpu
def test_engine_gpu():
    from mlrun_amd.models.llama import LlamaConfig

    check_engine_sgmv("cuda:0", LlamaConfig.tiny(
        num_layers=2, num_heads=4, num_kv_heads=2, hidden_size=512,
        intermediate_size=1024, vocab_size=2048))
