# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""The decode-step kernels, one op at a time, against the float64
references and bounds of tests/decode_refs.py (test_decode_kernels.py
shows on the CPU that a reference with one defect misses those bounds):
the slab consumers fused_add_rmsnorm_slab, swiglu_slab and rope_kv_slab,
attn_decode with bf16 and fp8 KV over every nsplit / group size / length
edge, and the fp8 activation path: quant_fp8_rows, the fp8 sidecar of
fused_add_rmsnorm and skinny_gemm_fp8.

Every operand is a slice of a buffer whose other elements are NaN (0x7F
for bytes, which is e4m3's NaN), outputs start as NaN, spare capacity is
NaN, and KV rows past a sequence's length are NaN: whatever is fetched
from outside a tensor, or left unwritten, shows.  The fences around
outputs must come back untouched.

MLRUN_ATTN_SCHUNK picks the 64-row instantiations of the attention
kernels and is read once per process, so `test_attn_decode_schunk64`
runs the attention cases in one child process with it set.

Largest error / bound measured on an MI355X: fused_add_rmsnorm_slab
0.99, swiglu_slab 1.00, rope_kv_slab 0.99, attn_decode 0.92 (bf16 KV) and
0.95 (fp8 KV) with 32-row and with 64-row chunks, identical for every
nsplit, fused_add_rmsnorm with the sidecar 0.94, its codes 0.94 and
quant_fp8_rows' codes 0.94 of the e4m3 half step, quant scales within
0.43 ulp, sidecar scales exact.  These bounds are the derived ones.
skinny_gemm_fp8 reached 19.7 times the derived bound at outputs that
cancel to 10^-4 of their terms: the fp8 MFMA does not accumulate in fp32.
Its bound carries a measured term, MFMA_FP8_ACC in decode_refs.py, the
one bound here that was set from a measurement (margin 2.3)."""

import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import decode_refs as R  # noqa: E402
from decode_refs import f64  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64        # fence elements on either side: keeps 16-byte alignment


class Fenced:
    """`values` (or NaN of that shape and dtype) on the GPU inside a
    flat buffer that is NaN (0x7F) everywhere else: PAD elements on both
    sides, and `spare` elements of NaN capacity behind the values that
    belong to `.all` but not to `.t`."""

    def __init__(self, values=None, shape=None, dtype=None, spare=0):
        if values is None:
            values = torch.full(shape, self.poison(dtype), dtype=dtype)
        n = values.numel()
        flat = torch.full((PAD + n + spare + PAD,),
                          self.poison(values.dtype), dtype=values.dtype)
        flat[PAD:PAD + n] = values.reshape(-1)
        self.buf = flat.cuda()
        self.n, self.spare = n, spare
        self.t = self.buf[PAD:PAD + n].view(values.shape)
        self.all = self.buf[PAD:PAD + n + spare]
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == 0

    @staticmethod
    def poison(dtype):
        return 0x7F if dtype == torch.uint8 else float("nan")

    def intact(self):
        """Nothing wrote outside the values."""
        outside = torch.cat([self.buf[:PAD], self.buf[PAD + self.n:]])
        if outside.dtype == torch.uint8:
            return bool((outside == 0x7F).all())
        return bool(torch.isnan(outside).all())


def _ext():
    import mlrun_amd._hip_ops as ext

    return ext


# -------------------------------------------------------- slab consumers

SLAB_HIDDEN = (64, 72, 1984, 2048, 2120)
KSPLITS = (2, 3, 8)


@requires_gpu
@pytest.mark.parametrize("ksplit", KSPLITS)
@pytest.mark.parametrize("hidden", SLAB_HIDDEN)
def test_fused_add_rmsnorm_slab(hidden, ksplit):
    """64 and 256 threads on both sides of hidden = 2048, and widths
    that are no multiple of 4 or 8 times the threads."""
    slabs, residual, weight = R.norm_slab_case(hidden, ksplit,
                                               hidden + ksplit)
    ref = R.norm_reference(f64(slabs), f64(residual), f64(weight))
    out = Fenced(shape=(3, hidden), dtype=torch.bfloat16)
    res = Fenced(residual)
    sl = Fenced(slabs, spare=hidden + 5)
    wt = Fenced(weight)
    _ext().fused_add_rmsnorm_slab(out.t, res.t, sl.all, wt.t, ksplit,
                                  R.NORM_EPS)
    torch.cuda.synchronize()
    what = f"fused_add_rmsnorm_slab hidden {hidden} ksplit {ksplit}"
    R.check(res.t, ref["z"], ref["z_bound"], what + " residual",
            "fused_add_rmsnorm_slab")
    R.check(out.t, ref["out"], ref["out_bound"], what,
            "fused_add_rmsnorm_slab")
    assert out.intact() and res.intact()


# the last case is grid-stride: rows * inter / 4 just exceeds 2048 * 256
SWIGLU_CASES = [(rows, inter, ks) for rows, inter in
                ((1, 4), (5, 132), (33, 1028)) for ks in KSPLITS] + \
    [(64, 32772, 2)]


@requires_gpu
@pytest.mark.parametrize("rows,inter,ksplit", SWIGLU_CASES)
def test_swiglu_slab(rows, inter, ksplit):
    slabs = R.swiglu_case(rows, inter, ksplit, rows + ksplit)
    ref = R.swiglu_reference(f64(slabs))
    out = Fenced(shape=(rows, inter), dtype=torch.bfloat16)
    sl = Fenced(slabs, spare=2 * inter + 3)
    _ext().swiglu_slab(out.t, sl.all, ksplit)
    torch.cuda.synchronize()
    R.check(out.t, ref["out"], ref["bound"],
            f"swiglu_slab {rows}x{inter} ksplit {ksplit}", "swiglu_slab")
    assert out.intact()


ROPE_CASES = [(hq, hkv, d, positions, pad)
              for hq, hkv in ((4, 2), (8, 1)) for d in (64, 128)
              for positions in ((0, 7, 15), (7, 7, 15)) for pad in (0, 64)]


@requires_gpu
@pytest.mark.parametrize("hq,hkv,d,positions,pad", ROPE_CASES)
def test_rope_kv_slab(hq, hkv, d, positions, pad):
    """q rows, Kc[pos] and Vc[pos] are right; every other cache row and
    the k / v / padding columns of the bf16 qkv buffer keep their bits."""
    from mlrun_amd import ops

    B, smax = 3, 16
    ksplit = KSPLITS[(hq + d // 64 + pad // 64 + positions[0]) % 3]
    slabs = R.rope_case(B, hq, hkv, d, ksplit, pad, hq + d + pad)
    qkv_row = slabs.shape[-1]
    pos = torch.tensor(positions, dtype=torch.int32)
    table = ops.build_rope_cos_sin(smax, d)
    ref = R.rope_reference(f64(slabs), pos, table, hq, hkv, d)
    qkv0 = R.sentinel_bf16(B, qkv_row)
    kc0 = R.sentinel_bf16(B, hkv, smax, d)
    vc0 = R.sentinel_bf16(B, hkv, smax, d).flip(0)
    qkv, kc, vc = Fenced(qkv0), Fenced(kc0), Fenced(vc0)
    sl = Fenced(slabs, spare=qkv_row + 7)
    cs = Fenced(table)
    _ext().rope_kv_slab(qkv.t, kc.t, vc.t, sl.all, pos.cuda(), cs.t, hq,
                        ksplit)
    torch.cuda.synchronize()
    what = f"rope_kv_slab {hq}/{hkv} d{d} {positions} pad {pad} " \
           f"ksplit {ksplit}"
    got_qkv, got_k, got_v = qkv.t.cpu(), kc.t.cpu(), vc.t.cpu()
    rows = torch.arange(B)
    R.check(got_qkv[:, :hq * d].view(B, hq, d), ref["q"]["ref"],
            ref["q"]["bound"], what + " q", "rope_kv_slab")
    R.check(got_k[rows, :, pos.long()], ref["k"]["ref"], ref["k"]["bound"],
            what + " k", "rope_kv_slab")
    R.check(got_v[rows, :, pos.long()], ref["v"]["ref"], ref["v"]["bound"],
            what + " v", "rope_kv_slab")
    assert R.same_bits(got_qkv[:, hq * d:], qkv0[:, hq * d:])
    got_k[rows, :, pos.long()] = kc0[rows, :, pos.long()]
    got_v[rows, :, pos.long()] = vc0[rows, :, pos.long()]
    assert R.same_bits(got_k, kc0) and R.same_bits(got_v, vc0)
    assert qkv.intact() and kc.intact() and vc.intact()


# ------------------------------------------------------------ attention

ATTN_CASES = [(G, lens, kv) for kv in ("bf16", "fp8") for G in R.GROUPS
              for lens in R.ATTN_LENS]
RAMPS = [(ramp, kv) for ramp in (0.02, -0.02) for kv in ("bf16", "fp8")]

_DEVICE = {}


def _attn_device(case):
    """The case's tensors on the GPU, once: q as a view into a
    [B, (Hq + 2 Hkv) D] buffer whose other columns are NaN, and as a
    contiguous tensor."""
    key = id(case)
    if key not in _DEVICE:
        B, Hq, _ = case["q"].shape
        width = (Hq + 2 * R.HKV) * R.D
        qkv = torch.full((B, width), float("nan"), dtype=torch.bfloat16)
        qkv[:, :Hq * R.D] = case["q"].reshape(B, Hq * R.D)
        qkv = Fenced(qkv)
        dev = dict(qkv=qkv, q=qkv.t[:, :Hq * R.D].view(B, Hq, R.D),
                   q_dense=Fenced(case["q"]), kc=Fenced(case["kc"]),
                   vc=Fenced(case["vc"]), lens=case["seq_lens"].cuda(),
                   k_scale=None, v_scale=None)
        assert not dev["q"].is_contiguous()
        if case["kv"] == "fp8":
            dev["k_scale"] = Fenced(case["k_scale"])
            dev["v_scale"] = Fenced(case["v_scale"])
        _DEVICE[key] = dev
    return _DEVICE[key]


def _attn_gpu(case, nsplit, dense=False):
    """One launch into a NaN output with a NaN workspace that has spare
    capacity; returns the output on the CPU."""
    dev = _attn_device(case)
    B, Hq, _ = case["q"].shape
    out = Fenced(shape=(B, Hq, R.D), dtype=torch.bfloat16)
    ws = None
    if nsplit > 1:
        ws = Fenced(shape=(B * Hq * nsplit * (R.D + 2),),
                    dtype=torch.float32, spare=R.D + 2)
    scales = [None if dev[s] is None else dev[s].t
              for s in ("k_scale", "v_scale")]
    _ext().attn_decode(out.t, dev["q_dense"].t if dense else dev["q"],
                       dev["kc"].t, dev["vc"].t, dev["lens"], R.ATTN_SCALE,
                       None if ws is None else ws.all, nsplit, *scales)
    torch.cuda.synchronize()
    assert out.intact() and (ws is None or ws.intact())
    return out.t.cpu()


def _check_attn(case, what, kernel, nsplits=R.NSPLITS):
    """Every nsplit is inside the bound, any two agree within twice the
    bound, and a sequence of length 0 gives exact zeros."""
    got = {}
    for nsplit in nsplits:
        got[nsplit] = _attn_gpu(case, nsplit)
        R.check(got[nsplit], case["ref"], case["bound"],
                f"{what} nsplit {nsplit}", kernel)
        for b, length in enumerate(case["lens"]):
            if length == 0:
                assert (got[nsplit][b] == 0).all(), f"{what}: len 0 != 0"
    first = got[nsplits[0]]
    for nsplit in nsplits[1:]:
        R.check(got[nsplit], f64(first), 2 * case["bound"],
                f"{what} nsplit {nsplit} against nsplit {nsplits[0]}")
    return got


@requires_gpu
@pytest.mark.parametrize("G,lens,kv", ATTN_CASES)
def test_attn_decode(G, lens, kv):
    """Lengths of exactly one chunk, one more, Smax, fewer than nsplit
    and 0, through the single kernel (nsplit 1) and the split one."""
    case = R.attn_case(G, lens, kv)
    _check_attn(case, f"attn_decode G {G} lens {lens} {kv}",
                f"attn_decode {kv}")


@requires_gpu
@pytest.mark.parametrize("ramp,kv", RAMPS)
def test_attn_decode_score_ramp(ramp, kv):
    """Scores that rise with the position raise the running max in
    every chunk and every split; falling ones leave it with the first
    (test_decode_kernels.py asserts both properties of the inputs)."""
    case = R.attn_case(4, R.RAMP_LENS, kv, ramp)
    _check_attn(case, f"attn_decode ramp {ramp} {kv}", f"attn_decode {kv}")


@requires_gpu
@pytest.mark.parametrize("kv", ("bf16", "fp8"))
def test_attn_decode_contiguous_q_and_repeat(kv):
    """A contiguous q gives the bits of the strided view, and the same
    call twice gives the same bits."""
    case = R.attn_case(4, R.ATTN_LENS[1], kv)
    for nsplit in (1, 3):
        strided = _attn_gpu(case, nsplit)
        assert R.same_bits(_attn_gpu(case, nsplit), strided)
        dense = _attn_gpu(case, nsplit, dense=True)
        R.check(dense, case["ref"], case["bound"],
                f"attn_decode contiguous q {kv} nsplit {nsplit}")
        assert R.same_bits(dense, strided)


def _run_attention_cases():
    for G, lens, kv in ATTN_CASES:
        _check_attn(R.attn_case(G, lens, kv),
                    f"attn_decode G {G} lens {lens} {kv}",
                    f"attn_decode {kv}")
    for ramp, kv in RAMPS:
        _check_attn(R.attn_case(4, R.RAMP_LENS, kv, ramp),
                    f"attn_decode ramp {ramp} {kv}", f"attn_decode {kv}")


@requires_gpu
def test_attn_decode_schunk64():
    """Every attention case above on the 64-row instantiations."""
    env = dict(os.environ, MLRUN_ATTN_SCHUNK="64")
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    proc = subprocess.run([sys.executable, os.path.abspath(__file__)],
                          cwd=REPO, env=env, capture_output=True, text=True,
                          timeout=300)
    print(proc.stdout[-600:])
    assert proc.returncode == 0 and "schunk ok 64" in proc.stdout, \
        f"{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}"


# -------------------------------------------------- fp8 activation path

SIDE_HIDDEN = (64, 1984, 2048, 2112)


@requires_gpu
@pytest.mark.parametrize("cols", SIDE_HIDDEN)
def test_quant_fp8_rows(cols):
    from mlrun_amd import ops

    a = R.quant_case(cols, cols)
    src = Fenced(a)
    codes = Fenced(shape=(3, cols), dtype=torch.uint8)
    scale = Fenced(shape=(3,), dtype=torch.float32)
    ops.quant_fp8_rows(src.t, codes.t, scale.t)
    torch.cuda.synchronize()
    R.check_quant(codes.t.cpu(), scale.t.cpu(), a, f"quant_fp8_rows {cols}",
                  "quant_fp8_rows")
    assert codes.intact() and scale.intact()


@requires_gpu
@pytest.mark.parametrize("with_residual", (True, False))
@pytest.mark.parametrize("hidden", SIDE_HIDDEN)
def test_fused_add_rmsnorm_fp8_sidecar(hidden, with_residual):
    """The bf16 output and new residual against float64; the sidecar's
    scale against amax|out| / 448 taken before the bf16 rounding; its
    codes, unswizzled and dequantized, against the bf16 output they
    encode.  Row 1 is all zero."""
    from mlrun_amd import ops

    x, residual, weight = R.norm_case(hidden, hidden,
                                      with_residual=with_residual)
    ref = R.norm_reference(f64(x)[None],
                           None if residual is None else f64(residual),
                           f64(weight))
    out = Fenced(shape=(3, hidden), dtype=torch.bfloat16)
    res = None if residual is None else Fenced(residual)
    codes = Fenced(shape=(3, hidden), dtype=torch.uint8)
    scale = Fenced(shape=(3,), dtype=torch.float32)
    ops.fused_add_rmsnorm(Fenced(x).t, Fenced(weight).t,
                          residual=None if res is None else res.t,
                          eps=R.NORM_EPS, out=out.t, out8=codes.t,
                          out_scale=scale.t)
    torch.cuda.synchronize()
    what = f"fused_add_rmsnorm sidecar {hidden} residual {with_residual}"
    R.check(out.t, ref["out"], ref["out_bound"], what, "fused_add_rmsnorm")
    if with_residual:
        R.check(res.t, ref["z"], ref["z_bound"], what + " residual",
                "fused_add_rmsnorm")
        assert res.intact()
    got_out, got_scale = out.t.cpu(), f64(scale.t)
    amax = ref["out"].abs().amax(-1)
    live = amax > 0
    want = amax[live] / R.FP8_MAX
    off = ((got_scale[live] - want).abs() / want).max().item() / R.R1
    print(f"scale off by {off:.3f} of 2^-8  {what}")
    assert off <= 1.0
    assert torch.isfinite(got_scale).all() and (got_scale > 0).all()
    plain = ops._fp8_pair_unswizzle(codes.t.cpu())
    assert (plain[~live] == 0).all() and (got_out[~live] == 0).all()
    ratio = R.fp8_code_ratio(plain, scale.t, got_out)
    R.MEASURED["fused_add_rmsnorm sidecar codes"] = max(
        R.MEASURED.get("fused_add_rmsnorm sidecar codes", 0.0), ratio)
    print(f"err/half-step {ratio:.3f}  {what}")
    assert ratio <= 1.0
    assert out.intact() and codes.intact() and scale.intact()


@requires_gpu
@pytest.mark.parametrize("k", R.GEMM_KS)
@pytest.mark.parametrize("m", R.GEMM_MS)
def test_skinny_gemm_fp8(m, k):
    """M = 17 and 33 are the first rows of the MT=2 and MT=4 classes,
    N = 80 is a ragged tile, K = 192 and 1088 leave wave and unroll
    tails, and ksplit 5 at K = 192 leaves two splits empty.  The scales
    have exactly M and N entries."""
    from mlrun_amd import ops

    a8, a_scale, w8, w_scale = R.gemm_fp8_case(m, k)
    dev = [Fenced(t) for t in (a8, a_scale, w8, w_scale)]
    for ksplit in R.GEMM_KSPLITS:
        ref, bound = R.gemm_fp8_reference(a8, a_scale, w8, w_scale, ksplit)
        out = Fenced(shape=(m, R.GEMM_N), dtype=torch.bfloat16)
        ws = Fenced(shape=(ksplit * m * R.GEMM_N,), dtype=torch.float32,
                    spare=R.GEMM_N + 1)
        ops.skinny_gemm_fp8(dev[0].t, dev[1].t, dev[2].t, dev[3].t,
                            out=out.t, c_f32=ws.all if ksplit > 1 else None,
                            ksplit=ksplit)
        torch.cuda.synchronize()
        R.check(out.t, ref, bound,
                f"skinny_gemm_fp8 M {m} K {k} ksplit {ksplit}",
                "skinny_gemm_fp8")
        assert out.intact() and ws.intact()


# ------------------------------------------------------- binding checks

def _raises(match, fn, *args):
    with pytest.raises(RuntimeError, match=match):
        fn(*args)


@requires_gpu
def test_rope_kv_slab_bad_arguments_raise_before_any_launch():
    from mlrun_amd import ops

    B, hq, hkv, d, smax, ksplit = 3, 4, 2, 64, 16, 2
    slabs = R.rope_case(B, hq, hkv, d, ksplit, 0, 1).cuda()
    qkv0 = R.sentinel_bf16(B, slabs.shape[-1])
    kc0 = R.sentinel_bf16(B, hkv, smax, d)
    qkv, kc, vc = qkv0.cuda(), kc0.cuda(), kc0.cuda()
    pos = torch.tensor([0, 7, 15], dtype=torch.int32).cuda()
    table = ops.build_rope_cos_sin(smax, d).cuda()
    fn = _ext().rope_kv_slab
    fn_args = [qkv, kc, vc, slabs, pos, table, hq, ksplit]

    def bad(match, index, value):
        args = list(fn_args)
        args[index] = value
        _raises(match, fn, *args)

    bad("vc must be on GPU", 2, kc0.clone())
    bad("vc must be bf16", 2, vc.float())
    bad("vc not contiguous", 2, vc.transpose(1, 2))
    bad("equal shape", 2, vc[:, :, :smax - 1].contiguous())
    bad(r"qkv must be \[B, rows\]", 0, qkv.view(B, hq + 2 * hkv, d))
    bad("positions size", 4, torch.zeros(B + 1, dtype=torch.int32,
                                         device="cuda"))
    bad("cos_sin must be", 5, ops.build_rope_cos_sin(smax, 2 * d).cuda())
    bad("ksplit must be at least 1", 7, 0)
    torch.cuda.synchronize()
    assert R.same_bits(qkv.cpu(), qkv0)
    assert R.same_bits(kc.cpu(), kc0) and R.same_bits(vc.cpu(), kc0)


@requires_gpu
def test_fused_add_rmsnorm_slab_bad_arguments_raise_before_any_launch():
    hidden, ksplit = 64, 2
    slabs, residual, weight = R.norm_slab_case(hidden, ksplit, 1)
    out = torch.full((3, hidden), float("nan"), dtype=torch.bfloat16,
                     device="cuda")
    res = residual.cuda()
    fn = _ext().fused_add_rmsnorm_slab
    _raises("residual size", fn, out, res[:2].contiguous(), slabs.cuda(),
            weight.cuda(), ksplit, R.NORM_EPS)
    _raises("weight size", fn, out, res, slabs.cuda(),
            torch.cat([weight, weight[:8]]).cuda(), ksplit, R.NORM_EPS)
    _raises("ksplit must be at least 1", fn, out, res, slabs.cuda(),
            weight.cuda(), 0, R.NORM_EPS)
    _raises("slabs too small", fn, out, res, slabs.cuda(), weight.cuda(),
            ksplit + 1, R.NORM_EPS)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and R.same_bits(res.cpu(), residual)


@requires_gpu
def test_swiglu_slab_bad_arguments_raise_before_any_launch():
    rows, inter, ksplit = 5, 132, 2
    slabs = R.swiglu_case(rows, inter, ksplit, 1).cuda()
    out = torch.full((rows, inter), float("nan"), dtype=torch.bfloat16,
                     device="cuda")
    fn = _ext().swiglu_slab
    _raises(r"out must be \[rows, inter\]", fn, out.view(-1), slabs, ksplit)
    _raises("ksplit must be at least 1", fn, out, slabs, 0)
    _raises("slabs too small", fn, out, slabs, ksplit + 1)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


@requires_gpu
def test_attn_decode_bad_arguments_raise_before_any_launch():
    case = R.attn_case(4, R.ATTN_LENS[1], "bf16")
    dev = _attn_device(case)
    B, Hq, _ = case["q"].shape
    out = torch.full((B, Hq, R.D), float("nan"), dtype=torch.bfloat16,
                     device="cuda")
    ws = torch.full((B * Hq * 1025 * (R.D + 2),), float("nan"),
                    device="cuda")
    kc, vc, lens = dev["kc"].t, dev["vc"].t, dev["lens"]
    fn = _ext().attn_decode
    _raises("vc shape must equal kc shape", fn, out, dev["q"], kc,
            vc[:, :, :R.SMAX - 1].contiguous(), lens, R.ATTN_SCALE, ws, 2)
    _raises("seq_lens must hold B entries", fn, out, dev["q"], kc, vc,
            torch.ones(B + 1, dtype=torch.int32, device="cuda"),
            R.ATTN_SCALE, ws, 2)
    for nsplit in (0, -1, 1025):
        _raises("bad nsplit", fn, out, dev["q"], kc, vc, lens,
                R.ATTN_SCALE, ws, nsplit)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(ws).all()


@requires_gpu
def test_measured_maxima_are_reported():
    """Runs last: prints the largest error / bound per kernel."""
    for name in sorted(R.MEASURED):
        print(f"measured {name}: {R.MEASURED[name]:.3f}")


if __name__ == "__main__":
    _run_attention_cases()
    for name in sorted(R.MEASURED):
        print(f"measured schunk64 {name}: {R.MEASURED[name]:.3f}")
    print("schunk ok", os.environ.get("MLRUN_ATTN_SCHUNK"))
