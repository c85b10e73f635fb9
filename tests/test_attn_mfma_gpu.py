# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""attn_prefill, attn_verify (+ its combine kernel) and rope_kv_varlen,
one op at a time, against the float64 references and the derived bound
of tests/attn_refs.py (test_attn_mfma.py shows on the CPU that a
reference with one defect leaves that bound on these very cases).

Outputs, caches, q and workspaces live in fenced buffers whose
surroundings and spare capacity are NaN.  Cache rows at and past a
sequence's end, and slots no live sequence uses, are NaN; q is a view
into a qkv buffer whose k / v columns are NaN.  Output rows the kernel
has to write start as NaN, rows it has to skip as distinct bit patterns
that must come back unchanged.

The cases: see PREFILL_SEQS, VERIFY_SHAPES and the other tables of
attn_refs.py.

Largest error / bound measured on an MI355X: attn_prefill 0.84,
attn_verify 0.78 (the same for every nsplit), rope_kv_varlen 0.99.
attn_verify with nsplit 1 and attn_prefill give the same bits on the
same chunk, for every shape of VERIFY_SHAPES."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_refs as A  # noqa: E402
import decode_refs as R  # noqa: E402
from gpu_fence import Fenced  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

D = A.D
PREFILL = [(heads, name) for heads in A.PREFILL_HEADS
           for name in A.PREFILL_SEQS]


def _ext():
    import mlrun_amd._hip_ops as ext

    return ext


_DEVICE = {}


def _device(case):
    """The case's tensors on the GPU, once: q as a view into a
    [T, (Hq + 2 Hkv) D] buffer whose other columns are NaN, and dense."""
    key = id(case)
    if key not in _DEVICE:
        T, Hq, Hkv = case["T"], case["Hq"], case["Hkv"]
        qkv = torch.full((T, (Hq + 2 * Hkv) * D), float("nan"),
                         dtype=torch.bfloat16)
        qkv[:, :Hq * D] = case["q"].reshape(T, Hq * D)
        qkv = Fenced(qkv)
        q = qkv.t[:, :Hq * D].view(T, Hq, D)
        assert not q.is_contiguous()
        _DEVICE[key] = dict(
            qkv=qkv, q=q, q_dense=Fenced(case["q"]), kc=Fenced(case["kc"]),
            vc=Fenced(case["vc"]), cu=case["cu_seqlens"].cuda(),
            slots=case["slots"].cuda(), kv_start=case["kv_start"].cuda())
    return _DEVICE[key]


def _fresh_out(case):
    """NaN in the rows the kernel writes, distinct bits in the others."""
    out = R.sentinel_bf16(case["T"], case["Hq"] * D)
    out[case["live"]] = float("nan")
    return out


def _finish(case, dev, out, ws=None):
    torch.cuda.synchronize()
    assert out.intact() and (ws is None or ws.intact())
    assert all(dev[name].intact() for name in ("qkv", "kc", "vc"))
    return out.t.cpu().view(case["T"], case["Hq"], D)


def _prefill_gpu(case, dense=False, max_q_len=None):
    dev = _device(case)
    out = Fenced(_fresh_out(case))
    _ext().attn_prefill(out.t, dev["q_dense"].t if dense else dev["q"],
                        dev["kc"].t, dev["vc"].t, dev["cu"], dev["slots"],
                        dev["kv_start"], A.SCALE,
                        case["max_q_len"] if max_q_len is None
                        else max_q_len)
    return _finish(case, dev, out)


def _verify_gpu(case, nsplit, dense=False):
    dev = _device(case)
    T, Hq = case["T"], case["Hq"]
    QL = case["seqs"][0][0]
    out = Fenced(_fresh_out(case))
    ws = None
    if nsplit > 1:
        from mlrun_amd import ops

        ws = Fenced(shape=(ops.attn_verify_ws_numel(T // QL, QL, Hq,
                                                    nsplit),),
                    dtype=torch.float32, spare=D + 5)
    q = dev["q_dense"].t if dense else dev["q"]
    _ext().attn_verify(out.t, q.view(T // QL, QL, Hq, D), dev["kc"].t,
                       dev["vc"].t, dev["kv_start"], A.SCALE,
                       None if ws is None else ws.all, nsplit)
    return _finish(case, dev, out, ws)


def _check(case, got, what, kernel, nsplit=1):
    """The rows of live sequences are inside the bound, the others keep
    their bits."""
    live = case["live"]
    R.check(got[live], case["ref"][live], A.bound(case, nsplit)[live],
            what, kernel)
    kept = _fresh_out(case).view_as(got)
    assert R.same_bits(got[~live], kept[~live]), \
        f"{what}: a skipped row was written"


# --------------------------------------------------------- attn_prefill

@requires_gpu
@pytest.mark.parametrize("heads,name", PREFILL)
def test_attn_prefill(heads, name):
    """Lengths around the 16-row wave and the 64-row block from start
    0, and chunks whose diagonal lies on every side of the mask and
    tile-skip predicates, one packed call each with the slots out of
    order; then the same call with max_q_len = T, whose surplus q-tiles
    exit."""
    case = A.prefill_case(heads, name)
    got = _prefill_gpu(case)
    _check(case, got, f"attn_prefill {heads} {name}", "attn_prefill")
    assert case["T"] > case["max_q_len"]
    assert R.same_bits(_prefill_gpu(case, max_q_len=case["T"]), got)


@requires_gpu
@pytest.mark.parametrize("seq", A.PREFILL_RAMP_SEQS)
@pytest.mark.parametrize("sign", (1, -1))
def test_attn_prefill_score_ramp(sign, seq):
    """Rising scores raise the running max in every tile and put the
    weight next to the diagonal; falling ones leave both at key 0."""
    case = A.prefill_ramp_case(sign, seq)
    _check(case, _prefill_gpu(case), f"attn_prefill ramp {sign} {seq}",
           "attn_prefill")


@requires_gpu
def test_attn_prefill_guards():
    """A zero-length sequence and sequences with slot -1, slot B and
    start -1 in one call: their rows keep their bits, the rows of the
    sequences between them are right."""
    case = A.prefill_guard_case()
    assert (~case["live"]).sum() == 9 + 7 + 5
    for max_q_len in (case["max_q_len"], case["T"]):
        _check(case, _prefill_gpu(case, max_q_len=max_q_len),
               f"attn_prefill guards max_q_len {max_q_len}", "attn_prefill")


@requires_gpu
def test_attn_prefill_contiguous_q_and_repeat():
    case = A.prefill_case((6, 2), "diagonal")
    strided = _prefill_gpu(case)
    assert R.same_bits(_prefill_gpu(case), strided)
    assert R.same_bits(_prefill_gpu(case, dense=True), strided)


# ---------------------------------------------------------- attn_verify

def _check_verify(case, what):
    """Every nsplit is inside the bound and any two agree within twice
    the bound."""
    live = case["live"]
    got = {}
    for nsplit in A.NSPLITS:
        got[nsplit] = _verify_gpu(case, nsplit)
        _check(case, got[nsplit], f"{what} nsplit {nsplit}", "attn_verify",
               nsplit)
    first = got[A.NSPLITS[0]]
    for nsplit in A.NSPLITS[1:]:
        R.check(got[nsplit][live], R.f64(first[live]),
                2 * A.bound(case, nsplit)[live],
                f"{what} nsplit {nsplit} against nsplit {A.NSPLITS[0]}")
    return got


@requires_gpu
@pytest.mark.parametrize("Hq,Hkv,QL", A.VERIFY_SHAPES)
def test_attn_verify(Hq, Hkv, QL):
    """base = 0, 1, 63, 64, 65, 200 and Smax - QL; G x QL = 1 .. 64
    columns, among them maps that are no power of two and cross a
    wave's 16 columns."""
    case = A.verify_case(Hq, Hkv, QL)
    _check_verify(case, f"attn_verify {Hq}/{Hkv} QL {QL}")


@requires_gpu
@pytest.mark.parametrize("sign", (1, -1))
def test_attn_verify_score_ramp(sign):
    case = A.verify_ramp_case(sign)
    _check_verify(case, f"attn_verify ramp {sign}")


@requires_gpu
def test_attn_verify_guards():
    """Rows with base -1 and base Smax - QL + 1 keep their bits in the
    single kernel and through the split and combine kernels."""
    case = A.verify_case(8, 2, 4, bases=A.verify_guard_bases(4))
    assert (~case["live"]).sum() == 8
    for nsplit in (1, 3):
        _check(case, _verify_gpu(case, nsplit),
               f"attn_verify guards nsplit {nsplit}", "attn_verify", nsplit)


@requires_gpu
def test_attn_verify_contiguous_q_and_repeat():
    case = A.verify_case(6, 2, 7)
    for nsplit in (1, 3):
        strided = _verify_gpu(case, nsplit)
        assert R.same_bits(_verify_gpu(case, nsplit), strided)
        assert R.same_bits(_verify_gpu(case, nsplit, dense=True), strided)


@requires_gpu
@pytest.mark.parametrize("Hq,Hkv,QL", A.VERIFY_SHAPES)
def test_attn_verify_nsplit_1_has_the_bits_of_attn_prefill(Hq, Hkv, QL):
    """The same chunk through both kernels (cu = QL * arange, kv_start =
    base): both run pf_tile over the same tiles with the same operands
    per column and share the epilogue."""
    case = A.verify_case(Hq, Hkv, QL)
    assert case["cu"] == [QL * b for b in range(len(case["seqs"]) + 1)]
    assert R.same_bits(_verify_gpu(case, 1), _prefill_gpu(case))


# ------------------------------------------------------- rope_kv_varlen

@requires_gpu
@pytest.mark.parametrize("d,smax,table_len", A.ROPE_CASES)
def test_rope_kv_varlen(d, smax, table_len):
    """37 tokens scattered over 3 slots in rows wider than the heads;
    tokens with slot -1, slot B, position -1, position Smax and a
    position past the cos/sin table are skipped."""
    case = A.rope_varlen_case(d, smax, table_len)
    qkv, kc, vc = Fenced(case["qkv"]), Fenced(case["kc"]), Fenced(case["vc"])
    table = Fenced(case["table"])
    _ext().rope_kv_varlen(qkv.t, kc.t, vc.t, case["pos"].cuda(),
                          case["slot"].cuda(), table.t, A.ROPE_HQ)
    torch.cuda.synchronize()
    A.check_rope_varlen(case, qkv.t.cpu(), kc.t.cpu(), vc.t.cpu(),
                        f"rope_kv_varlen d{d} smax {smax} table {table_len}",
                        "rope_kv_varlen")
    assert qkv.intact() and kc.intact() and vc.intact()


# ------------------------------------------------------- binding checks

def _bad(fn, fn_args, match, index, value):
    args = list(fn_args)
    args[index] = value
    with pytest.raises(RuntimeError, match=match):
        fn(*args)


def _offset_q(q):
    """q's values at a view that starts 4 elements (8 bytes) into its
    buffer."""
    flat = torch.zeros(q.numel() + 8, dtype=q.dtype, device=q.device)
    flat[4:4 + q.numel()] = q.reshape(-1)
    return flat[4:4 + q.numel()].view(q.shape)


@requires_gpu
def test_attn_prefill_bad_arguments_raise_before_any_launch():
    case = A.prefill_case((8, 2), "lengths")
    dev = _device(case)
    T, Hq = case["T"], case["Hq"]
    out0 = R.sentinel_bf16(T, Hq * D)
    out = out0.cuda()
    kc, vc, q = dev["kc"].t, dev["vc"].t, dev["q_dense"].t
    kc0, vc0 = kc.clone(), vc.clone()
    fn = _ext().attn_prefill
    args = [out, q, kc, vc, dev["cu"], dev["slots"], dev["kv_start"],
            A.SCALE, case["max_q_len"]]
    _bad(fn, args, "must be bf16", 1, q.float())
    _bad(fn, args, "must be bf16", 3, vc.float())
    _bad(fn, args, "must be int32", 5, dev["slots"].long())
    _bad(fn, args, "not contiguous", 2, kc.transpose(1, 2))
    _bad(fn, args, "equal shape", 3, vc[:, :, :A.SMAX - 1].contiguous())
    _bad(fn, args, "16-byte aligned", 1, _offset_q(q))
    _bad(fn, args, "cu_seqlens", 4, dev["cu"][:-1].contiguous())
    _bad(fn, args, "cu_seqlens", 6, dev["kv_start"][:-1].contiguous())
    _bad(fn, args, "bad max_q_len", 8, T + 1)
    _bad(fn, args, "bad max_q_len", 8, -1)
    _bad(fn, args, r"out must be \[T, Hq\*D\]", 0, out[:-1])
    wide = torch.zeros(T, 32, D, dtype=torch.bfloat16, device="cuda")
    _bad(fn, [torch.zeros(T, 32 * D, dtype=torch.bfloat16, device="cuda"),
              wide] + args[2:], "grouped heads", 1, wide)      # G 16
    torch.cuda.synchronize()
    assert R.same_bits(out.cpu(), out0)
    assert R.same_bits(kc.cpu(), kc0.cpu()) and \
        R.same_bits(vc.cpu(), vc0.cpu())


@requires_gpu
def test_attn_verify_bad_arguments_raise_before_any_launch():
    from mlrun_amd import ops

    case = A.verify_case(8, 2, 4)
    dev = _device(case)
    T, Hq, QL = case["T"], case["Hq"], 4
    B = T // QL
    out0 = R.sentinel_bf16(T, Hq * D)
    out = out0.cuda()
    kc, vc = dev["kc"].t, dev["vc"].t
    kc0, vc0 = kc.clone(), vc.clone()
    q = dev["q_dense"].t.view(B, QL, Hq, D)
    need = ops.attn_verify_ws_numel(B, QL, Hq, 3)
    ws = torch.full((need + 4,), float("nan"), device="cuda")
    fn = _ext().attn_verify
    args = [out, q, kc, vc, dev["kv_start"], A.SCALE, ws, 3]
    _bad(fn, args, "must be bf16", 1, q.float())
    _bad(fn, args, "must be bf16", 2, kc.float())
    _bad(fn, args, "must be int32", 4, dev["kv_start"].long())
    _bad(fn, args, "not contiguous", 3, vc.transpose(1, 2))
    _bad(fn, args, "16-byte aligned", 1, _offset_q(q))
    _bad(fn, args, "agree on B", 4, dev["kv_start"][:-1].contiguous())
    _bad(fn, args, "partial_ws too small", 6, ws[:need - 1])
    _bad(fn, args, "partial_ws must be 16-byte aligned", 6, ws[1:need + 1])
    _bad(fn, args, "must be f32", 6, ws.double())
    _bad(fn, args, "needs partial_ws", 6, None)
    _bad(fn, args, "bad nsplit", 7, 0)
    _bad(fn, args, "bad nsplit", 7, 1025)
    q9 = torch.zeros(B, 9, Hq, D, dtype=torch.bfloat16, device="cuda")
    _bad(fn, args, "1 <= QL <= 8", 1, q9)
    q16 = torch.zeros(B, QL, 32, D, dtype=torch.bfloat16, device="cuda")
    _bad(fn, args, "grouped heads", 1, q16)                     # G 16
    torch.cuda.synchronize()
    assert R.same_bits(out.cpu(), out0) and torch.isnan(ws).all()
    assert R.same_bits(kc.cpu(), kc0.cpu()) and \
        R.same_bits(vc.cpu(), vc0.cpu())


@requires_gpu
def test_rope_kv_varlen_bad_arguments_raise_before_any_launch():
    from mlrun_amd import ops

    d, smax, table_len = A.ROPE_CASES[0]
    case = A.rope_varlen_case(d, smax, table_len)
    qkv, kc, vc = case["qkv"].cuda(), case["kc"].cuda(), case["vc"].cuda()
    pos, slot = case["pos"].cuda(), case["slot"].cuda()
    table = case["table"].cuda()
    fn = _ext().rope_kv_varlen
    args = [qkv, kc, vc, pos, slot, table, A.ROPE_HQ]
    _bad(fn, args, "must be bf16", 0, qkv.float())
    _bad(fn, args, "must be bf16", 2, vc.float())
    _bad(fn, args, "must be int32", 3, pos.long())
    _bad(fn, args, "must be f32", 5, table.double())
    _bad(fn, args, "not contiguous", 1, kc.transpose(1, 2))
    _bad(fn, args, "not contiguous", 0, qkv[:, :-8])
    _bad(fn, args, "equal shape", 2, vc[:, :, :smax - 1].contiguous())
    _bad(fn, args, "one entry per token", 3, pos[:-1].contiguous())
    _bad(fn, args, "one entry per token", 4, torch.cat([slot, slot[:1]]))
    _bad(fn, args, "qkv row too small", 6, A.ROPE_HQ + 1)
    _bad(fn, args, "cos_sin must be",
         5, ops.build_rope_cos_sin(table_len, 2 * d).cuda())
    torch.cuda.synchronize()
    assert R.same_bits(qkv.cpu(), case["qkv"])
    assert R.same_bits(kc.cpu(), case["kc"]) and \
        R.same_bits(vc.cpu(), case["vc"])


@requires_gpu
def test_measured_maxima_are_reported():
    """Runs last: prints the largest error / bound per kernel."""
    for name in sorted(R.MEASURED):
        print(f"measured {name}: {R.MEASURED[name]:.3f}")
