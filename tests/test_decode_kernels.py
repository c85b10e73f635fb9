# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""The bounds of tests/decode_refs.py mean something, shown without a
GPU: on the inputs test_decode_kernels_gpu.py uses, the CPU branches of
`ops` stay inside them against the float64 references, and a reference
with one deliberate defect falls outside by a clear factor (MUTATION).

Largest error / bound of the CPU branches: attn_decode 0.92 (bf16 KV)
and 0.97 (fp8 KV), fused_add_rmsnorm 0.65 (of r = 3 * 2^-9, which is 0.98
of 2^-8), swiglu_fused 1.00, rope_kv_fused 0.99, skinny_gemm_fp8 0.98,
quant_fp8_rows 0.94 of the e4m3 half step with the scales within 0.5 ulp.
The smallest mutant is 7.6 times its bound (a dropped KV row at L = 129)."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import decode_refs as R  # noqa: E402
from decode_refs import f64  # noqa: E402

# a mutated reference must miss the bound by at least this factor
MUTATION = 5.0

ATTN_CASES = [(G, lens, kv) for kv in ("bf16", "fp8") for G in R.GROUPS
              for lens in R.ATTN_LENS]
RAMPS = [(ramp, kv) for ramp in (0.02, -0.02) for kv in ("bf16", "fp8")]
SIDE_HIDDEN = (64, 1984, 2048, 2112)
SLAB_HIDDEN = (64, 72, 1984, 2048, 2120)
KSPLITS = (2, 3, 8)
# the last case is grid-stride: rows * inter / 4 just exceeds 2048 * 256
SWIGLU_CASES = [(rows, inter, ks) for rows, inter in
                ((1, 4), (5, 132), (33, 1028)) for ks in KSPLITS] + \
    [(64, 32772, 2)]
ROPE_SHAPES = [(hq, hkv, d) for hq, hkv in ((4, 2), (8, 1))
               for d in (64, 128)]
ROPE_POSITIONS = ((0, 7, 15), (7, 7, 15))


def _mutated(ref, bound, mutant, what):
    ratio = R.worst(mutant, ref, bound)
    print(f"mutant err/bound {ratio:.1f}  {what}")
    assert ratio >= MUTATION, f"{what}: mutant only {ratio:.2f} x the bound"


# ------------------------------------------------------------ attention

def _cpu_attn(case):
    """ops.attn_decode's CPU branch on the case (rows >= len hold NaN,
    so reading one shows)."""
    from mlrun_amd import ops

    return ops.attn_decode(case["q"], case["kc"], case["vc"],
                           case["seq_lens"], k_scale=case["k_scale"],
                           v_scale=case["v_scale"])


@pytest.mark.parametrize("G,lens,kv", ATTN_CASES)
def test_attn_decode_cpu_branch(G, lens, kv):
    case = R.attn_case(G, lens, kv)
    got = _cpu_attn(case)
    ref = case["ref"]
    if kv == "fp8":     # the CPU branch does not stage the rows as bf16
        ref = R.attn_reference(f64(case["q"]), case["keys_exact"],
                               case["vals_exact"], lens)
    R.check(got, ref, R.attn_bound(ref), f"attn_decode cpu {G} {lens} {kv}",
            f"attn_decode cpu {kv}")
    for b, length in enumerate(lens):
        if length == 0:
            assert (got[b] == 0).all()


@pytest.mark.parametrize("ramp,kv", RAMPS)
def test_attn_ramp_cases_move_the_running_max(ramp, kv):
    """Rising scores: every chunk of 32 or 64 rows raises the running
    max, for every head.  Falling scores: the first chunk holds it."""
    case = R.attn_case(4, R.RAMP_LENS, kv, ramp)
    ref = case["ref"] if kv == "bf16" else R.attn_reference(
        f64(case["q"]), case["keys_exact"], case["vals_exact"], R.RAMP_LENS)
    R.check(_cpu_attn(case), ref, R.attn_bound(ref),
            f"attn_decode cpu ramp {ramp} {kv}")
    for chunk in (32, 64):
        for b in range(3):
            for h in range(8):
                m = R.chunk_maxima(case, b, h, chunk)
                if ramp > 0:
                    assert all(x < y for x, y in zip(m, m[1:])), (b, h, m)
                else:
                    assert all(m[0] > y for y in m[1:]), (b, h, m)


@pytest.mark.parametrize("G,lens,kv", ATTN_CASES)
def test_attn_dropped_row_is_seen(G, lens, kv):
    """Leaving any one of the first, middle and last KV row out of any
    sequence moves some output of every head off the reference by
    MUTATION times its bound."""
    case = R.attn_case(G, lens, kv)
    q = f64(case["q"])
    for b, length in enumerate(lens):
        if length < 2:
            continue
        for row in sorted({0, length // 2, length - 1}):
            mutant = R.attn_reference(q, case["keys"], case["vals"], lens,
                                      drop=(b, row))
            for h in range(q.shape[1]):
                ratio = R.worst(mutant[b, h], case["ref"][b, h],
                                case["bound"][b, h])
                assert ratio >= MUTATION, (b, h, row, ratio)


# ---------------------------------------------------------------- norms

@pytest.mark.parametrize("with_residual", (True, False))
@pytest.mark.parametrize("hidden", SIDE_HIDDEN + (72, 2120))
def test_fused_add_rmsnorm_cpu_branch(hidden, with_residual):
    from mlrun_amd import ops

    x, residual, weight = R.norm_case(hidden, hidden, with_residual=
                                      with_residual)
    ref = R.norm_reference(f64(x)[None],
                           None if residual is None else f64(residual),
                           f64(weight))
    new_res = None if residual is None else residual.clone()
    out = ops.fused_add_rmsnorm(x, weight, residual=new_res,
                                eps=R.NORM_EPS)
    what = f"fused_add_rmsnorm cpu {hidden} {with_residual}"
    R.check(out, ref["out"], ref["out_bound"], what,
            "fused_add_rmsnorm cpu")
    if with_residual:
        R.check(new_res, ref["z"], ref["z_bound"], what + " residual")
    assert (out[1] == 0).all()


@pytest.mark.parametrize("ksplit", KSPLITS)
@pytest.mark.parametrize("hidden", SLAB_HIDDEN)
def test_norm_slab_left_out_is_seen(hidden, ksplit):
    slabs, residual, weight = R.norm_slab_case(hidden, ksplit,
                                               hidden + ksplit)
    args = (f64(slabs), f64(residual), f64(weight))
    ref = R.norm_reference(*args)
    for skip in (0, ksplit - 1):
        mutant = R.norm_reference(*args, skip=skip)
        what = f"norm slab {skip} of {ksplit} left out, hidden {hidden}"
        _mutated(ref["out"], ref["out_bound"], mutant["out"], what)
        _mutated(ref["z"], ref["z_bound"], mutant["z"], what + " residual")


# --------------------------------------------------------------- swiglu

@pytest.mark.parametrize("rows,inter,ksplit", SWIGLU_CASES)
def test_swiglu_cpu_branch_and_mutants(rows, inter, ksplit):
    from mlrun_amd import ops

    slabs = R.swiglu_case(rows, inter, ksplit, rows + ksplit)
    ref = R.swiglu_reference(f64(slabs))
    total = f64(slabs).sum(0)
    span = total[:, :inter]
    assert span.min() <= -11.99 and span.max() >= 11.99
    # the CPU branch takes the bf16 gate|up buffer: one "slab"
    gu = total.float().to(torch.bfloat16)
    own = R.swiglu_reference(f64(gu)[None])
    R.check(ops.swiglu_fused(gu), own["out"], own["bound"],
            f"swiglu_fused cpu {rows}x{inter}", "swiglu_fused cpu")
    what = f"swiglu {rows}x{inter} ks{ksplit}"
    _mutated(ref["out"], ref["bound"],
             R.swiglu_reference(f64(slabs), swap=True)["out"],
             what + " gate/up swapped")
    for skip in (0, ksplit - 1):
        _mutated(ref["out"], ref["bound"],
                 R.swiglu_reference(f64(slabs), skip=skip)["out"],
                 what + f" slab {skip} left out")


# ----------------------------------------------------------------- rope

@pytest.mark.parametrize("positions", ROPE_POSITIONS)
@pytest.mark.parametrize("hq,hkv,d", ROPE_SHAPES)
def test_rope_kv_fused_cpu_branch_and_mutants(hq, hkv, d, positions):
    from mlrun_amd import ops

    B, smax, ksplit = 3, 16, 3
    slabs = R.rope_case(B, hq, hkv, d, ksplit, 64, hq + d)
    pos = torch.tensor(positions, dtype=torch.int32)
    table = ops.build_rope_cos_sin(smax, d)
    ref = R.rope_reference(f64(slabs), pos, table, hq, hkv, d)
    what = f"rope {hq}/{hkv} d{d} {positions}"
    flipped = R.rope_reference(f64(slabs), pos, table, hq, hkv, d,
                               sign=-1.0)
    if any(positions):      # position 0 rotates by nothing
        for part in ("q", "k"):
            live = [b for b, p in enumerate(positions) if p]
            _mutated(ref[part]["ref"][live], ref[part]["bound"][live],
                     flipped[part]["ref"][live], what + f" sign, {part}")
    left_out = R.rope_reference(f64(slabs), pos, table, hq, hkv, d, skip=1)
    for part in ("q", "k", "v"):
        _mutated(ref[part]["ref"], ref[part]["bound"],
                 left_out[part]["ref"], what + f" slab left out, {part}")

    # the CPU branch takes the bf16 qkv buffer: one "slab"
    qkv = f64(slabs).sum(0).float().to(torch.bfloat16)
    own = R.rope_reference(f64(qkv)[None], pos, table, hq, hkv, d)
    kc = R.sentinel_bf16(B, hkv, smax, d)
    vc = R.sentinel_bf16(B, hkv, smax, d)
    kc0, vc0 = kc.clone(), vc.clone()
    ops.rope_kv_fused(qkv, kc, vc, pos, table, hq)
    rows = torch.arange(B)
    R.check(qkv[:, :hq * d].view(B, hq, d), own["q"]["ref"],
            own["q"]["bound"], what + " cpu q", "rope_kv_fused cpu")
    R.check(kc[rows, :, pos.long()], own["k"]["ref"], own["k"]["bound"],
            what + " cpu k", "rope_kv_fused cpu")
    R.check(vc[rows, :, pos.long()], own["v"]["ref"], own["v"]["bound"],
            what + " cpu v", "rope_kv_fused cpu")
    kc[rows, :, pos.long()] = kc0[rows, :, pos.long()]
    vc[rows, :, pos.long()] = vc0[rows, :, pos.long()]
    assert R.same_bits(kc, kc0) and R.same_bits(vc, vc0)


# ------------------------------------------------------------------ fp8

@pytest.mark.parametrize("cols", SIDE_HIDDEN)
def test_quant_fp8_rows_cpu_branch_and_moved_group(cols):
    from mlrun_amd import ops

    a = R.quant_case(cols, cols)
    codes, scale = ops.quant_fp8_rows(a)
    R.check_quant(codes, scale, a, f"quant_fp8_rows cpu {cols}",
                  "quant_fp8_rows cpu")
    # one 8-byte group of the pair swizzle moved to its neighbour's place
    moved = codes.clone()
    moved[0, 0:8], moved[0, 8:16] = codes[0, 8:16], codes[0, 0:8]
    ratio = R.fp8_code_ratio(ops._fp8_pair_unswizzle(moved), scale, a)
    print(f"moved group err/half-step {ratio:.1f}")
    assert ratio >= MUTATION


@pytest.mark.parametrize("k", R.GEMM_KS)
@pytest.mark.parametrize("m", R.GEMM_MS)
def test_skinny_gemm_fp8_cpu_branch_and_shifted_scale(m, k):
    from mlrun_amd import ops

    a8, a_scale, w8, w_scale = R.gemm_fp8_case(m, k)
    ref, bound = R.gemm_fp8_reference(a8, a_scale, w8, w_scale, 1,
                                      mfma=False)
    got = ops.skinny_gemm_fp8(a8, a_scale, w8, w_scale)
    R.check(got, ref, bound, f"skinny_gemm_fp8 cpu M{m} K{k}",
            "skinny_gemm_fp8 cpu")
    # the mutant is held to the bound the GPU test uses
    ref, bound = R.gemm_fp8_reference(a8, a_scale, w8, w_scale, 5)
    if m > 1:
        mutant, _ = R.gemm_fp8_reference(a8, a_scale, w8, w_scale, 1,
                                         shift_scale=True)
        for row in range(m):
            ratio = R.worst(mutant[row], ref[row], bound[row])
            assert ratio >= MUTATION, (row, ratio)


def test_measured_maxima_are_reported():
    """Runs last: prints the largest error / bound per CPU branch."""
    for name in sorted(R.MEASURED):
        print(f"{name}: {R.MEASURED[name]:.3f}")
