# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""The bound of tests/attn_refs.py means something, shown without a GPU
on the cases test_attn_mfma_gpu.py runs:

* E, the relative fp32 error of a softmax weight, is at most R1 / 2 on
  every row of every case (0.05 R1 on the N(0,1) cases, 0.49 R1 on the
  ramps), so the first-order bound holds;
* a simulation of the tile loop's arithmetic (fp32 tiles of 64, bf16 P,
  fp32 l, every nsplit) stays inside the bound: at most 0.84 of it;
* the CPU branches of ops.attn_prefill and ops.attn_verify stay inside
  it, and skip what the kernels skip, as ops.rope_kv_varlen does;
* a float64 reference with one defect leaves it.  On the N(0,1) cases
  every mutant that applies reaches MUTATION times the bound somewhere in
  every sequence it touches.  On the ramp cases (RAMP = 0.04) every
  mutant of the ramp reaches it on every (row, head) pair it touches; the
  smallest figure is 4.2 (the leak at length 200 from start 40).

The leak, the dropped diagonal and a start off by one (which for every
row is one of those two) show on the rising ramp, where the newest keys
carry the weight; the dropped key 0 on the falling one.  On the other
ramp the key in question weighs e^-0.23 per row of distance and is
invisible, which is why there are two.  The first key of a 64-tile shows
on the N(0,1) cases only; on the rising ramp it is the dropped diagonal
of the rows at 64, 128, ...

Trial before the cases were fixed: at RAMP = 0.02 and lengths up to 259
the leak reached 1.9 times the bound at the worst row; at +-0.04 and
lengths 2..259 the leak reached 21, the dropped diagonal 16 and the
dropped key 0 37 times at the worst row through its best head, with
E / R1 <= 0.5.  A steeper ramp would break E <= R1 / 2 at 240 keys.  On
every single (row, head) pair, four sequences of eight heads in one call
with seed 0 gave 1.6 (leak), 1.8 (diagonal) and 2.9 (key 0) at the worst
of 5280 pairs, 0.04 % to 0.35 % of them under MUTATION: the N(0,1) part of
a score (standard deviation 1.1) against a ramp step of 0.23.  Hence one
sequence per ramp case and a chosen seed, see attn_refs.RAMP_SEEDS."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_refs as A  # noqa: E402
import decode_refs as R  # noqa: E402

# a mutated reference must miss the bound by at least this factor
MUTATION = 4.0

PREFILL = [(heads, name) for heads in A.PREFILL_HEADS
           for name in A.PREFILL_SEQS]
MASK_MUTANTS = ("leak", "no_diagonal", "no_key0", "no_tile_first",
                "start+1", "start-1")
RAMP_MUTANTS = {1: ("leak", "no_diagonal", "start+1", "start-1"),
                -1: ("no_key0",)}


def _plain_cases():
    for heads, name in PREFILL:
        yield f"prefill {heads} {name}", A.prefill_case(heads, name)
    yield "prefill guards", A.prefill_guard_case()
    for shape in A.VERIFY_SHAPES:
        yield f"verify {shape}", A.verify_case(*shape)
    yield "verify guards", A.verify_case(
        8, 2, 4, bases=A.verify_guard_bases(4))


def _ramp_cases():
    for sign in (1, -1):
        for seq in A.PREFILL_RAMP_SEQS:
            yield f"prefill ramp {sign} {seq}", sign, \
                A.prefill_ramp_case(sign, seq)
        yield f"verify ramp {sign}", sign, A.verify_ramp_case(sign)


def _all_cases():
    yield from _plain_cases()
    for what, _, case in _ramp_cases():
        yield what, case


def _nsplits(case):
    return A.NSPLITS if case["rule"] == "verify" else (1,)


def test_weight_error_is_at_most_half_a_bf16_rounding():
    """E <= R1 / 2 on every row; and the bound is a function of the
    case alone: it has the same bits before and after the code under
    test ran on the case."""
    for what, case in _all_cases():
        live = case["live"]
        worst = (case["E"][live].max() / R.R1).item()
        print(f"E / R1 {worst:.3f}  {what}")
        assert worst <= 0.5, what
        before = A.bound(case)
        A.simulate(case)
        _cpu_op(case)
        assert torch.equal(before, A.bound(case))
        assert torch.isfinite(before[live]).all() and (before[live] > 0).all()


def test_simulated_tile_loop_is_inside_the_bound():
    for what, case in _all_cases():
        live = case["live"]
        for nsplit in _nsplits(case):
            R.check(A.simulate(case, nsplit)[live], case["ref"][live],
                    A.bound(case, nsplit)[live],
                    f"simulation {what} nsplit {nsplit}", "simulation")


def _cpu_op(case, out=None):
    from mlrun_amd import ops

    T, Hq = case["T"], case["Hq"]
    if out is None:
        out = R.sentinel_bf16(T, Hq * A.D)
    if case["rule"] == "verify":
        QL = case["seqs"][0][0]
        ops.attn_verify(case["q"].view(-1, QL, Hq, A.D), case["kc"],
                        case["vc"], case["kv_start"], out=out)
    else:
        ops.attn_prefill(case["q"], case["kc"], case["vc"],
                         case["cu_seqlens"], case["slots"],
                         case["kv_start"], out=out)
    return out.view(T, Hq, A.D)


def test_cpu_branches_are_inside_the_bound_and_skip_what_the_kernels_skip():
    """The caches hold NaN wherever no live sequence has a row, so a
    read of a skipped sequence's slot, or past an end, shows; the rows
    of a skipped sequence keep their bits."""
    for what, case in _all_cases():
        live = case["live"]
        got = _cpu_op(case)
        R.check(got[live], case["ref"][live], A.bound(case)[live],
                f"cpu {what}", f"attn_{case['rule']} cpu")
        before = R.sentinel_bf16(case["T"], case["Hq"] * A.D).view_as(got)
        assert R.same_bits(got[~live], before[~live]), what
    assert (~A.prefill_guard_case()["live"]).sum() == 9 + 7 + 5
    assert (~A.verify_case(8, 2, 4, bases=A.verify_guard_bases(4))["live"]
            ).sum() == 8


def test_cpu_attn_prefill_clamps_rows_past_T_and_skips_a_negative_row0():
    from mlrun_amd import ops

    case = A.prefill_case((2, 2), "lengths")
    out = R.sentinel_bf16(case["T"], 2 * A.D)
    cu = case["cu_seqlens"].clone()
    cu[0], cu[-1] = -1, case["T"] + 5
    ops.attn_prefill(case["q"], case["kc"], case["vc"], cu, case["slots"],
                     case["kv_start"], out=out)
    got = out.view(case["T"], 2, A.D)
    first = case["cu"][1]
    assert R.same_bits(got[:first], R.sentinel_bf16(
        case["T"], 2 * A.D).view_as(got)[:first])
    R.check(got[first:], case["ref"][first:], A.bound(case)[first:],
            "cpu prefill, cu_seqlens past T")


@pytest.mark.parametrize("d,smax,table_len", A.ROPE_CASES)
def test_cpu_rope_kv_varlen_skips_what_the_kernel_skips(d, smax, table_len):
    from mlrun_amd import ops

    case = A.rope_varlen_case(d, smax, table_len)
    qkv, kc, vc = case["qkv"].clone(), case["kc"].clone(), case["vc"].clone()
    ops.rope_kv_varlen(qkv, kc, vc, case["pos"], case["slot"],
                       case["table"], A.ROPE_HQ)
    A.check_rope_varlen(case, qkv, kc, vc,
                        f"rope_kv_varlen cpu d{d} smax {smax}",
                        "rope_kv_varlen cpu")


def _sequences(case, touched):
    for i in range(len(case["seqs"])):
        rows = slice(case["cu"][i], case["cu"][i + 1])
        if touched[rows].any():
            yield i, rows


def test_plain_cases_see_every_mutant_in_every_sequence():
    for what, case in _plain_cases():
        for name in A.MUTANTS:
            out, touched = A.mutant(case, name)
            if out is None or not touched.any():
                continue
            ratio = A.margins(case, out, touched)
            worst = min(ratio[rows].max().item()
                        for _, rows in _sequences(case, touched))
            print(f"mutant err/bound {worst:.1f}  {what} {name}")
            for i, rows in _sequences(case, touched):
                assert ratio[rows].max() >= MUTATION, \
                    (what, name, case["seqs"][i], ratio[rows].max())


def test_ramp_cases_see_every_mutant_on_every_row_of_every_head():
    """Every (row, head) pair a mutant of the ramp touches is off by
    MUTATION times the bound; a mask mutant touches all rows but the one
    at position 0 (the diagonal, key 0) or at Smax - 1 (the leak)."""
    for what, sign, case in _ramp_cases():
        for name in RAMP_MUTANTS[sign] + ("head_mod", "swap_gj"):
            out, touched = A.mutant(case, name)
            if out is None:
                assert name == "swap_gj" and case["rule"] == "prefill"
                continue
            ratio = A.margins(case, out, touched)[touched]
            print(f"mutant err/bound {ratio.min():.2f} at the worst of "
                  f"{ratio.numel()} (row, head) pairs  {what} {name}")
            if name in MASK_MUTANTS:
                assert touched.all(-1).sum() >= case["T"] - 1
            else:
                assert touched.any()
            assert ratio.min() >= MUTATION, (what, name)


def test_measured_maxima_are_reported():
    """Runs last: prints the largest error / bound per code path."""
    for name in sorted(R.MEASURED):
        print(f"{name}: {R.MEASURED[name]:.3f}")
